"""CPU tests of utils/coco_eval.py, the numpy specification of COCO's bounding-box evaluation: bbox_iou on boxes where
every intermediate is exact, match_segment against a literal restatement of COCOeval.evaluateImg (tests/_coco_cases.py)
and on hand-worked segments, accumulate / summarize on data sets small enough to work by hand, the annotation reader on
tests/golden/coco/instances_tiny.json and the results file's round trip."""
import json
import os

import numpy as np
import pytest

import _coco_cases as K
from tensorflow_yolo2_amd.utils import coco_eval as CE

EPS = np.spacing(1)


# ---------------------------------------------------------------- bbox_iou
def test_bbox_iou_exact_cases():
    assert CE.bbox_iou([3, 4, 10, 6], [3, 4, 10, 6], False) == 1.0                  # identical
    assert CE.bbox_iou([0, 0, 4, 4], [10, 10, 4, 4], False) == 0.0                  # disjoint
    assert CE.bbox_iou([0, 0, 4, 4], [4, 0, 4, 4], False) == 0.0                    # touching: ow = 0
    assert CE.bbox_iou([0, 0, 4, 4], [0, 4, 4, 4], False) == 0.0                    # touching: oh = 0
    assert CE.bbox_iou([0, 0, 2, 2], [0, 0, 2, 1], False) == 0.5                    # 2 / ((4 + 2) - 2)
    assert CE.bbox_iou([0, 0, 4, 4], [2, 2, 4, 4], False) == 4.0 / 28.0
    # the crowd form: the union is the detection's area, whatever the region's
    assert CE.bbox_iou([2, 2, 2, 2], [0, 0, 100, 100], True) == 1.0
    assert CE.bbox_iou([0, 0, 4, 4], [2, 0, 100, 100], True) == 0.5
    assert CE.bbox_iou([0, 0, 4, 4], [2, 0, 100, 100], False) == 8.0 / ((16.0 + 10000.0) - 8.0)
    # and 0.5 matches at the threshold 0.5
    rows = K.rows_from_xywh([[0, 0, 2, 2]], [1], 0)
    word = CE.match_segment(rows, [[0, 0, 2, 1, 1]], [2], [0], [0.5, 0.5 + 2 ** -40], [[0, 1e10]])
    assert word.tolist() == [[1]]                                                   # a true positive at 0.5 alone


def test_row_forms_give_the_same_boxes():
    xywh = np.array([[0, 0, 20, 20], [30, 17, 5, 1], [100, 2, 300, 77]], np.float64)
    for form in (0, 1):
        assert np.array_equal(CE.row_xywh(K.rows_from_xywh(xywh, [1, 2, 3], form), form), xywh)
    assert K.rows_from_xywh(xywh, [1, 2, 3], 0)[0].tolist() == [1, 1, 20, 20, 1, 0]   # 1-based inclusive corners
    f = K.rows_from_xywh([[0.5, 1.25, 20.5, 3]], [1], 1)[:, :4].view(np.float32)[0].tolist()
    assert f == [1.5, 2.25, 22.0, 5.25]                                             # both corners carry the + 1
    with pytest.raises(ValueError, match="row_form 2"):
        CE.row_xywh(np.zeros((1, 6), np.int32), 2)


# ---------------------------------------------------------------- match_segment
@pytest.mark.parametrize("row_form", [0, 1])
def test_match_segment_equals_the_literal_evaluate_img(row_form):
    rng = np.random.default_rng(2014 + row_form)
    seen = set()
    for _ in range(150):
        rows, gt, area, crowd = K.random_segment(rng, row_form)
        got = CE.match_segment(rows, gt, area, crowd, row_form=row_form)
        want = K.evaluate_img_literal(rows, gt, area, crowd, CE.THRESHOLDS, CE.AREA_RANGES, row_form)
        assert got.dtype == np.int32 and got.shape == (len(rows), 4)
        assert np.array_equal(got, want)
        assert not (got >> 20).any()                                                # the other bits are 0
        seen.update(np.unique(CE.match_values(got, 10)).tolist())
    assert seen == {0, 1, 2}
    # other thresholds and ranges, T = 1 and A = 1 among them
    for thresholds, ranges in (([0.5], [[0, 1e10]]), (np.linspace(0.05, 0.8, 16), [[0, 2000], [100, 1e5], [0, 50], [64, 64]])):
        for _ in range(20):
            rows, gt, area, crowd = K.random_segment(rng, row_form)
            assert np.array_equal(CE.match_segment(rows, gt, area, crowd, thresholds, ranges, row_form),
                                  K.evaluate_img_literal(rows, gt, area, crowd, thresholds, ranges, row_form))


@pytest.mark.parametrize("row_form", [0, 1])
@pytest.mark.parametrize("case", K.HAND, ids=[c[0] for c in K.HAND])
def test_match_segment_hand_worked(case, row_form):
    rows, gt, area, crowd, thresholds, ranges, expect = K.hand_case(case, row_form)
    assert np.array_equal(CE.match_segment(rows, gt, area, crowd, thresholds, ranges, row_form), expect)


def test_match_segment_limits():
    rows = K.rows_from_xywh([[0, 0, 2, 2]], [1], 0)
    for thresholds, ranges in ((np.linspace(0.1, 0.9, 17), None), (None, [[0, 1]] * 5), ([], None)):
        with pytest.raises(ValueError, match="at most 16 and 4"):
            CE.match_segment(rows, np.zeros((0, 5)), [], [], thresholds, ranges)


# ---------------------------------------------------------------- accumulate / summarize
def test_detections_equal_to_the_ground_truths_score_one(golden_dir):
    ds = CE.read_instances(os.path.join(golden_dir, "coco", "instances_tiny.json"))
    segments = []
    for e, im in enumerate(ds["images"]):
        for c in range(3):
            boxes = [o["bbox"] for o in im["anns"] if o["category"] == c]
            if boxes:
                segments.append((e, c, boxes, np.linspace(0.9, 0.6, len(boxes))))
    rows = K.spec_rows(ds, segments, 1)                       # float rows: the file's boxes have halves and quarters
    precision, recall = CE.accumulate(rows, ds)
    stats = CE.summarize(precision, recall)
    assert precision.shape == (10, 101, 3, 4, 3) and recall.shape == (10, 3, 4, 3)
    assert abs(stats[0] - 1.0) < 1e-12 and abs(stats[8] - 1.0) < 1e-12             # AP, AR100
    assert all(abs(s - 1.0) < 1e-12 for s in stats[:6] + stats[8:])                # every size occurs in the file
    crowd_row = np.nonzero((rows["class"] == 2) & (rows["image"] == 2))[0]         # the crowd region's own box: ignored
    assert rows["match"][crowd_row].tolist() == [[K.ALL_IG] * 4]


def test_a_category_without_ground_truth_stays_out_of_the_mean():
    ds = K.make_dataset([(1, [(0, 0, 100, 100, 0, 10000, 0)])])
    rows = K.spec_rows(ds, [(0, 0, [[0, 0, 100, 100]], [0.9]), (0, 1, [[0, 0, 100, 100], [5, 5, 50, 50]], [0.8, 0.7])], 0)
    precision, recall = CE.accumulate(rows, ds)
    assert np.all(precision[:, :, 1] == -1) and np.all(recall[:, 1] == -1)
    assert np.all(precision[:, :, 0, 1:3] == -1)              # no small and no medium object either
    stats = CE.summarize(precision, recall)
    assert abs(stats[0] - 1.0) < 1e-12 and stats[3] == stats[4] == -1.0 and abs(stats[5] - 1.0) < 1e-12
    # a category WITH ground truth and no row: recall 0, precision 0 at every recall point
    none = {k: v[:0] for k, v in rows.items()}
    precision, recall = CE.accumulate(none, ds)
    assert np.all(precision[:, :, 0, 0] == 0) and np.all(recall[:, 0, 0] == 0)
    assert CE.summarize(precision, recall)[0] == 0.0


def test_hand_computed_curve_and_max_dets():
    # one image, two large objects of category 0; rows in descending score: A exactly, a box far away, B exactly
    ds = K.make_dataset([(5, [(0, 0, 100, 100, 0, 10000, 0), (200, 0, 100, 100, 0, 10000, 0)])])
    rows = K.spec_rows(ds, [(0, 0, [[0, 0, 100, 100], [0, 300, 100, 100], [200, 0, 100, 100]], [0.9, 0.8, 0.7])], 0)
    assert rows["match"].tolist() == [[K.ALL_TP, K.ALL_IG, K.ALL_IG, K.ALL_TP], [0, K.ALL_IG, K.ALL_IG, 0],
                                      [K.ALL_TP, K.ALL_IG, K.ALL_IG, K.ALL_TP]]
    precision, recall = CE.accumulate(rows, ds)
    # tp = 1, 1, 2; fp = 0, 1, 1; recall 0.5, 0.5, 1; precision 1, 1/2, 2/3 -> from the back 1, 2/3, 2/3
    p_first, p_last = 1.0 / (1.0 + EPS), 2.0 / (3.0 + EPS)
    curve = np.array([p_first] * 51 + [p_last] * 50)          # recall points 0 .. 0.50, then 0.51 .. 1
    for t in range(10):
        assert np.array_equal(precision[t, :, 0, 0, 2], curve)
        assert np.array_equal(precision[t, :, 0, 3, 2], curve)
    ap = (51 * p_first + 50 * p_last) / 101
    stats = CE.summarize(precision, recall)
    assert all(abs(stats[i] - ap) < 1e-15 for i in (0, 1, 2, 5)) and stats[3] == stats[4] == -1.0
    # maxDets: with one row per image only A is found, with ten both
    assert stats[6] == 0.5 and stats[7] == stats[8] == 1.0 and stats[11] == 1.0
    assert np.array_equal(precision[0, :, 0, 0, 0], np.array([p_first] * 51 + [0.0] * 50))


def test_equal_scores_keep_image_id_order():
    # the image of the lower id holds the false positive: it goes first, tp = 0, 1 and fp = 1, 1
    ds = K.make_dataset([(9, [(0, 0, 50, 50, 0, 2500, 0)]), (4, [(0, 0, 50, 50, 0, 2500, 0)])])
    assert [im["id"] for im in ds["images"]] == [4, 9]
    rows = K.spec_rows(ds, [(0, 0, [[200, 200, 50, 50]], [0.5]), (1, 0, [[0, 0, 50, 50]], [0.5])], 0)
    precision, recall = CE.accumulate(rows, ds)
    half = 1.0 / (2.0 + EPS)
    assert np.array_equal(precision[0, :, 0, 0, 2], np.array([half] * 51 + [0.0] * 50))
    assert recall[0, 0, 0, 2] == 0.5
    with pytest.raises(ValueError, match="segment order"):
        CE.accumulate({k: v[::-1] for k, v in rows.items()}, ds)


def test_summary_lines_are_cocos():
    lines = CE.summary_lines([0.5] * 12)
    assert len(lines) == 12
    assert lines[0] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.500"
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.500"
    assert lines[6] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500"
    assert lines[11] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = 0.500"


# ---------------------------------------------------------------- the files
def test_read_instances(golden_dir, tmp_path):
    path = os.path.join(golden_dir, "coco", "instances_tiny.json")
    ds = CE.read_instances(path)
    assert ds["categories"] == [1, 3, 17] and ds["names"] == ["person", "car", "cat"]
    assert [im["id"] for im in ds["images"]] == [7, 19, 42]
    assert [im["file_name"] for im in ds["images"]] == ["testImg1.jpg", "testImg1.jpg", "testImg2.jpg"]
    assert (ds["images"][0]["width"], ds["images"][0]["height"]) == (352, 240)
    assert [len(im["anns"]) for im in ds["images"]] == [3, 0, 4]                    # the empty image is kept
    assert [o["category"] for o in ds["images"][0]["anns"]] == [1, 2, 0]            # file order, indices by sorted id
    anns = ds["images"][2]["anns"]
    assert [o["category"] for o in anns] == [0, 1, 2, 0]
    assert [o["iscrowd"] for o in anns] == [0, 0, 1, 0]                             # a missing iscrowd is 0
    assert anns[3]["area"] == 400.25 and anns[3]["bbox"] == [300.0, 20.0, 20.5, 30.0]
    # a Darknet list file restricts by base name
    listing = tmp_path / "5k.txt"
    listing.write_text("/data/coco/images/val2014/testImg2.jpg\n\n")
    assert [im["id"] for im in CE.read_instances(path, str(listing))["images"]] == [42]
    listing.write_text("val2014/testImg1.jpg\n")
    assert [im["id"] for im in CE.read_instances(path, str(listing))["images"]] == [7, 19]
    listing.write_text("val2014/elsewhere.jpg\n")
    with pytest.raises(ValueError, match="instances_tiny.json.*elsewhere.jpg"):
        CE.read_instances(path, str(listing))
    # errors name the file
    data = json.load(open(path))
    for name, change, text in (("noimages.json", lambda d: d.pop("images"), "no COCO instances file"),
                               ("badimage.json", lambda d: d["annotations"][0].update(image_id=5), "image id 5"),
                               ("badcat.json", lambda d: d["annotations"][1].update(category_id=2), "category id 2"),
                               ("nobbox.json", lambda d: d["annotations"][2].pop("bbox"), "malformed record")):
        d = json.loads(json.dumps(data))
        change(d)
        bad = tmp_path / name
        bad.write_text(json.dumps(d))
        with pytest.raises(ValueError, match=name + ".*" + text):
            CE.read_instances(str(bad))
    text = tmp_path / "text.json"
    text.write_text("not json")
    with pytest.raises(ValueError, match="text.json: not a JSON file"):
        CE.read_instances(str(text))
    with pytest.raises(OSError):
        CE.read_instances(str(tmp_path / "missing.json"))


def test_write_results_round_trip(golden_dir, tmp_path):
    ds = CE.read_instances(os.path.join(golden_dir, "coco", "instances_tiny.json"))
    rows = K.spec_rows(ds, [(0, 1, [[40, 50, 150, 100]], [0.75]), (2, 0, [[30.5, 60.25, 200, 380.5], [1, 2, 3, 4]], [0.5, 0.25]),
                            (2, 2, [[10, 10, 300, 200]], [0.125])], 1)
    path = CE.write_results(str(tmp_path / "results.json"), rows, ds)
    back = json.load(open(path))
    assert back == [{"image_id": 7, "category_id": 3, "bbox": [40.0, 50.0, 150.0, 100.0], "score": 0.75},
                    {"image_id": 42, "category_id": 1, "bbox": [30.5, 60.25, 200.0, 380.5], "score": 0.5},
                    {"image_id": 42, "category_id": 1, "bbox": [1.0, 2.0, 3.0, 4.0], "score": 0.25},
                    {"image_id": 42, "category_id": 17, "bbox": [10.0, 10.0, 300.0, 200.0], "score": 0.125}]
    assert '"bbox":[40.000000, 50.000000, 150.000000, 100.000000], "score":0.750000}' in open(path).read()
    empty = CE.write_results(str(tmp_path / "empty.json"), {k: v[:0] for k, v in rows.items()}, ds)
    assert json.load(open(empty)) == []
