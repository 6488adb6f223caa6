"""One detection row per (candidate, class), as Darknet's `valid` writes them: utils/detect_batch.anchor_detect_classes
(the specification of y2_detect_anchor_classes_batch), the reuse of match_image over (image, class) segments against
the devkit's protocol (utils/voc_eval.voc_map), and the devkit's results files.  No GPU: the last but one test checks
that the specification alone, on the heads tests/test_gpu_detect_anchor_classes.py sends to the kernel, meets what
makes per-class rows differ from per-anchor rows."""
import os

import numpy as np
import pytest

from test_gpu_detect_anchor import ANCHORS, SHAPES, _anchor_case
from tensorflow_yolo2_amd.utils import detect_batch as DB
from tensorflow_yolo2_amd.utils import voc_eval

SCORE_THRESH, IOU_THRESH, MAX_PER_CLASS = 0.02, 0.45, 8


def test_one_class_is_anchor_detect():
    from oracle import ext_ref as X
    S, B, C = 7, 3, 1
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    boxes, scores = X.decode_anchors(net, ANCHORS[:B])
    assert scores.shape == (3, K, 1)
    for img, max_out in ((0, MAX_PER_CLASS), (1, MAX_PER_CLASS), (2, MAX_PER_CLASS), (0, K)):
        h, w = SHAPES[img]
        det, score, count = DB.anchor_detect_classes(boxes[img], scores[img], w, h, SCORE_THRESH, IOU_THRESH, max_out)
        want_det, want_score = DB.anchor_detect(boxes[img], scores[img][:, 0], np.zeros(K, np.int64), w, h,
                                                SCORE_THRESH, IOU_THRESH, max_out)
        c = len(want_det)
        assert det.shape == (1, max_out, 6) and score.shape == (1, max_out) and count.tolist() == [c]
        assert det.dtype == np.int32 and score.dtype == np.float32 and count.dtype == np.int32
        assert np.array_equal(det[0, :c], want_det)
        assert np.array_equal(score[0, :c].view(np.uint32), want_score.view(np.uint32))
        assert (det[0, c:] == -1).all() and (score[0, c:] == 0).all()
    assert c > MAX_PER_CLASS                                              # the uncapped call kept more than the cap


def _relative(box, w, h):
    """the (cx, cy, w, h) relative to a w x h image whose anchor_candidates box is the 1-based inclusive `box`"""
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    return ((x0 - 1 + bw // 2 + 0.5) / w, (y0 - 1 + bh // 2 + 0.5) / h, (bw + 0.5) / w, (bh + 0.5) / h)


# three hand-made images of 400 x 300 and three classes.  Every candidate: (1-based pixel box, scores of the 3 classes)
HAND_W, HAND_H = 400, 300
HAND_GT = (
    # image 0: an object of class 0 that two detections cover, a difficult object of class 1
    [((101, 101, 200, 200), 0, 0), ((251, 51, 350, 150), 1, 1)],
    # image 1: two objects of class 0 (one segment, two objects), one of class 2
    [((21, 21, 120, 120), 0, 0), ((201, 21, 300, 120), 0, 0), ((151, 171, 250, 270), 2, 0)],
    # image 2: nothing of class 0 or 2: every detection there is a false positive
    [((51, 51, 150, 150), 1, 0)],
)
HAND_CAND = (
    [((101, 101, 200, 170), (0.90, 0.30, 0.0)),      # IoU 0.7 with the object: true positive; also a class-1 row
     ((101, 131, 200, 200), (0.80, 0.0, 0.0)),       # IoU 0.7 with the same object, 0.4 with the row above: a duplicate
     ((251, 51, 350, 150), (0.0, 0.70, 0.25)),       # the difficult object: ignored in class 1, a miss in class 2
     ((1, 201, 60, 300), (0.50, 0.0, 0.0))],         # nowhere near anything
    [((21, 21, 120, 120), (0.90, 0.0, 0.40)),        # equal to image 0's best score: the order across images counts
     ((201, 31, 300, 130), (0.50, 0.0, 0.0)),
     ((151, 171, 250, 270), (0.60, 0.0, 0.80)),      # class 2's object; its class-0 row is a false positive
     ((26, 21, 125, 120), (0.85, 0.0, 0.0))],        # IoU 0.9 with the first: suppressed
    [((51, 51, 150, 150), (0.50, 0.95, 0.0)),        # 0.50: equal scores across images in class 0 as well
     ((201, 101, 300, 250), (0.30, 0.0, 0.0))],
)


def test_segment_matching_agrees_with_the_devkit_protocol():
    """match_image per (image, class) segment + map_from_flags over the flattened rows = voc_eval.voc_map of the same
    detections, as floats: a ground-truth object has one class, so its `taken` bit is only ever met in its class's
    segment, and a row's flag depends on earlier rows of its own image and class alone"""
    n, C, M = len(HAND_CAND), 3, 4
    dets, scores, counts, flags = [], [], [], []
    devkit_det, devkit_gt = [], []
    for img in range(n):
        boxes = np.array([_relative(b, HAND_W, HAND_H) for b, _s in HAND_CAND[img]], np.float32)
        sc = np.array([s for _b, s in HAND_CAND[img]], np.float32)
        det, score, count = DB.anchor_detect_classes(boxes, sc, HAND_W, HAND_H, 0.1, IOU_THRESH, M)
        gt = np.array([b + (c,) for b, c, _d in HAND_GT[img]], np.float64)
        difficult = [d for _b, _c, d in HAND_GT[img]]
        flag = np.full((C, M), -1, np.int32)
        for c in range(C):
            flag[c, :count[c]] = DB.match_image(det[c, :count[c]], gt, difficult, 0.5)
            for k in range(count[c]):
                assert det[c, k, 4] == c
                devkit_det.append((img, c, float(score[c, k])) + tuple(int(v) for v in det[c, k, :4]))
        devkit_gt += [(img, c) + b + (d,) for b, c, d in HAND_GT[img]]
        dets.append(det), scores.append(score), counts.append(count), flags.append(flag)
    # the hand-made boxes came through the decode as intended, and every case is present
    assert dets[0][0, :3, :4].tolist() == [list(HAND_CAND[0][k][0]) for k in (0, 1, 3)]
    assert flags[0][0].tolist() == [1, 0, 0, -1]                          # two detections on one object: the second misses
    assert flags[0][1, :2].tolist() == [2, 0]                             # the difficult object, then a row off it
    assert counts[1].tolist() == [3, 0, 2] and 3 not in dets[1][0, :, 5]  # a suppressed candidate, an empty segment
    assert sorted(flags[1][0, :3].tolist()) == [0, 1, 1]                  # a class holding two objects
    assert scores[0][0, 0] == scores[1][0, 0] and scores[0][0, 2] == scores[1][0, 2] == scores[2][0, 0]
    rows = DB.class_rows(np.stack(dets), np.stack(scores), np.stack(counts), np.stack(flags))
    assert len(rows[0]) == len(devkit_det) == int(np.stack(counts).sum())
    assert [(c, s) for (_i, c, s, *_b) in devkit_det] == list(zip(rows[0].tolist(), rows[1].tolist()))
    npos = DB.npos_from_objects([c for g in HAND_GT for _b, c, _d in g], [d for g in HAND_GT for _b, _c, d in g])
    assert npos == {0: 3, 1: 1, 2: 1}
    for use_07 in (True, False):
        got = DB.map_from_flags(rows, npos, use_07_metric=use_07)
        want = voc_eval.voc_map(devkit_det, devkit_gt, num_class=C, iou_thresh=0.5, use_07_metric=use_07)
        assert got == want, (use_07, got, want)
        assert 0.0 < got[0] < 1.0 and sorted(got[1]) == [0, 1, 2]


def _segments(S, B, C, max_per_class):
    from oracle import ext_ref as X
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    assert K not in (64, 128, 256, 512, 1024, 2048)
    boxes, scores = X.decode_anchors(net, ANCHORS[:B])
    out = []
    for img in range(3):
        h, w = SHAPES[img]
        valid = np.stack([DB.anchor_candidates(boxes[img], scores[img][:, c], np.full(K, c), w, h, SCORE_THRESH)[0]
                          for c in range(C)], axis=1)                     # [K][C]
        det, score, count = DB.anchor_detect_classes(boxes[img], scores[img], w, h, SCORE_THRESH, IOU_THRESH,
                                                     max_per_class)
        with np.errstate(all="ignore"):
            argmax = scores[img].argmax(axis=1)
        live = np.arange(max_per_class)[None, :] < count[:, None]
        off_best = int((argmax[det[live][:, 5]] != det[live][:, 4]).sum())
        out.append({"valid": valid, "count": count, "off_best": off_best})
    return out


@pytest.mark.parametrize("S,B,C", ((13, 5, 20), (19, 5, 20)))
def test_inputs_exercise_what_per_class_rows_add(S, B, C):
    """at threshold 0.02, IoU 0.45: anchors valid in two classes and more, kept rows of a class that is not the anchor's
    best, suppressed candidates, segments that reach the cap (images 0 and 2) and images without a row (image 1)"""
    K = S * S * B
    capped = _segments(S, B, C, MAX_PER_CLASS)
    full = _segments(S, B, C, K)
    multi = int((capped[0]["valid"].sum(axis=1) >= 2).sum())
    suppressed = int(full[0]["valid"].sum() - full[0]["count"].sum())
    print("(%d, %d, %d) image 0: %d anchors valid in >= 2 classes, %d suppressed, %d keeps off the best class (%d under "
          "the cap)" % (S, B, C, multi, suppressed, full[0]["off_best"], capped[0]["off_best"]))
    assert multi >= K // 2
    assert suppressed >= K and full[0]["off_best"] >= K
    assert capped[0]["off_best"] > 0
    assert (full[0]["count"] > MAX_PER_CLASS).all()                       # the cap cuts rows off in every class
    for img in (0, 2):
        assert (capped[img]["count"] == MAX_PER_CLASS).all()              # 20 of 20 segments saturated
    assert not capped[1]["valid"].any() and (capped[1]["count"] == 0).all()
    assert (full[2]["valid"].sum(axis=0) > 64).all()                      # the sort is wider than one wave ...
    assert (full[0]["valid"].sum(axis=0) < K // 2).all()                  # ... and much narrower than K


def test_single_cell_has_short_segments():
    """(1, 5, 20): five candidates; segments that are neither empty nor at the cap, and an empty one beside them"""
    seg = _segments(1, 5, 20, MAX_PER_CLASS)[0]
    count = seg["count"]
    assert int((seg["valid"].sum(axis=1) >= 2).sum()) == 5                # every anchor is valid in several classes
    assert ((count > 0) & (count < MAX_PER_CLASS)).any() and (count < MAX_PER_CLASS).all() and (count == 0).any()
    assert int(seg["valid"].sum() - count.sum()) > 0                      # and some are suppressed


def test_results_files_parse_back(tmp_path):
    rng = np.random.default_rng(5)
    ids = ["2007_%06d" % k for k in (3, 11, 12, 40)]
    names = ("aeroplane", "bicycle", "bird")
    N = 40
    rows = {"image": np.sort(rng.integers(0, 3, N)), "class": rng.integers(0, 2, N),       # no row of image 3, of bird
            "score": rng.uniform(0.005, 1.0, N).astype(np.float32), "box": rng.integers(1, 500, (N, 4)).astype(np.int32)}
    out = str(tmp_path / "results" / "VOC2007" / "Main")
    paths = voc_eval.write_results_files(out, "test", ids, names, rows)
    assert [os.path.basename(p) for p in paths] == ["comp4_det_test_%s.txt" % c for c in names]
    assert sorted(os.listdir(out)) == sorted(os.path.basename(p) for p in paths)
    seen = 0
    for c, path in enumerate(paths):
        with open(path) as f:
            lines = [line.split() for line in f.read().splitlines()]
        sel = np.nonzero(rows["class"] == c)[0]
        assert len(lines) == len(sel)
        for line, k in zip(lines, sel):                                   # one line per row, in the rows' order
            assert len(line) == 6 and line[0] == ids[rows["image"][k]]
            assert abs(float(line[1]) - float(rows["score"][k])) <= 0.5e-6
            assert [int(v) for v in line[2:]] == rows["box"][k].tolist()
        seen += len(lines)
    assert seen == N and os.path.getsize(paths[2]) == 0
