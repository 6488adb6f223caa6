"""COCO evaluation on the device: y2_coco_match_batch (csrc/coco.hip) bit for bit against utils/coco_eval.match_segment per
segment, its buffer behaviour and argument errors, engine.coco_match_batch's contract, coco/coco_eval_yolov2.py end to end
on tests/golden/coco/instances_tiny.json with a random `.weights` file of tests/golden/cfg/narrow-tiny-coco.cfg, and the
ground truths scored as their own detections."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _coco_cases as K
import _darknet_ref as R
from tensorflow_yolo2_amd.utils import coco_eval as CE

gpu = pytest.mark.gpu
NCLS, ENTRIES = 4, 3                           # 12 segments: every entry named once per class


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def tables(max_obj, row_form, rng):
    """the box / area / crowd / count tables of three entries: entry 0 holds random objects of classes 1..3 (none of class
    4), entry 1 is FULL of objects of class 1 (with max_obj = 70, more than a wave has lanes), entry 2 holds crowd regions
    only.  The slots beyond an entry's count hold objects that would match if they were read"""
    step = 8 if row_form == 0 else 8.5
    boxes = np.zeros((ENTRIES, max_obj, 5))
    boxes[:, :, 0:2] = rng.integers(0, 8, (ENTRIES, max_obj, 2)) * step
    boxes[:, :, 2:4] = rng.integers(1, 7, (ENTRIES, max_obj, 2)) * step
    boxes[:, :, 4] = rng.integers(1, NCLS, (ENTRIES, max_obj))
    boxes[1, :, 4] = 1
    area = boxes[:, :, 2] * boxes[:, :, 3] * rng.choice([1.0, 0.5, 0.25, 4.0, 8.0], (ENTRIES, max_obj))
    crowd = (rng.random((ENTRIES, max_obj)) < 0.2).astype(np.uint8)
    crowd[2] = 1
    counts = np.array([max(1, max_obj - 2), max_obj, max(1, max_obj // 2)], np.int32)
    return boxes, area, crowd, counts


def segments(boxes, counts, max_out, row_form, rng, mixed):
    """det int32 [12][max_out][6] (-1 beyond count), count [12], index [12].  Segment 0 is empty, segment 4 (entry 1,
    class 1: the full entry) is full, segment 3 is class 4 of entry 0 (no ground truth of the class); the rows are the
    entry's objects, moved by whole grid steps or not at all, and boxes of their own.  mixed: some rows of a segment carry
    another class than the segment's, as the rows of a per-image detector would"""
    step = 8 if row_form == 0 else 8.5
    n = ENTRIES * NCLS
    det = np.full((n, max_out, 6), -1, np.int32)
    count = rng.integers(0, min(max_out, 12) + 1, n).astype(np.int32)
    count[0], count[4], count[3] = 0, max_out, max(count[3], 1)
    index = np.repeat(np.arange(ENTRIES), NCLS).astype(np.int32)
    for s in range(n):
        e, c = index[s], s % NCLS + 1
        xywh, cls = np.zeros((count[s], 4)), np.full(count[s], c)
        for k in range(count[s]):
            own = np.nonzero(boxes[e, :counts[e], 4] == c)[0]
            if len(own) and rng.random() < 0.75:
                xywh[k] = boxes[e, rng.choice(own), :4]
                xywh[k, :2] = np.maximum(xywh[k, :2] + rng.integers(-1, 2, 2) * step * (rng.random() < 0.4), 0)
                xywh[k, 2:] = np.maximum(xywh[k, 2:] + rng.integers(-1, 2, 2) * step * (rng.random() < 0.3), step)
            else:
                xywh[k, :2] = rng.integers(0, 8, 2) * step
                xywh[k, 2:] = rng.integers(1, 7, 2) * step
            if mixed and rng.random() < 0.3:
                cls[k] = rng.integers(1, NCLS + 1)
        det[s, :count[s]] = K.rows_from_xywh(xywh, cls, row_form)
    return det, count, index


def expected(det, count, index, tabs, thresholds, ranges, row_form):
    boxes, area, crowd, counts = tabs
    A = len(CE.AREA_RANGES if ranges is None else ranges)
    want = np.full(det.shape[:2] + (A,), -1, np.int32)
    for s in range(len(det)):
        e, m = index[s], counts[index[s]]
        want[s, :count[s]] = CE.match_segment(det[s, :count[s]], boxes[e, :m], area[e, :m], crowd[e, :m], thresholds, ranges,
                                              row_form)
    return want


SHAPES = [(1, 1), (5, 8), (70, 100)]                                      # (max_obj, max_out)
LIMITS = {"coco": (None, None), "one": ([0.5], [[0, 1e10]]),
          "most": (np.linspace(0.05, 0.8, 16), [[0, 2000], [100, 1e5], [0, 50], [64, 64]])}


@gpu
@pytest.mark.parametrize("row_form", [0, 1])
@pytest.mark.parametrize("limits", sorted(LIMITS))
@pytest.mark.parametrize("max_obj,max_out", SHAPES)
def test_match_is_bit_equal_to_match_segment(max_obj, max_out, limits, row_form):
    import torch
    from tensorflow_yolo2_amd import engine as E
    thresholds, ranges = LIMITS[limits]
    rng = np.random.default_rng(1000 * max_obj + 10 * row_form + len(limits))
    tabs = tables(max_obj, row_form, rng)
    det, count, index = segments(tabs[0], tabs[3], max_out, row_form, rng, mixed=limits == "most")
    want = expected(det, count, index, tabs, thresholds, ranges, row_form)
    A = want.shape[2]
    out = torch.full((len(det), max_out, A), 0x7fc00000, dtype=torch.int32, device="cuda")     # NaN bit patterns
    args = (dev(det), dev(count)) + tuple(dev(t) for t in tabs) + (dev(index), thresholds, ranges, row_form)
    got = E.coco_match_batch(*args, out=out)
    assert got is out
    first = host(got)
    assert np.array_equal(first, want)
    assert np.all(first[np.arange(max_out)[None, :] >= count[:, None]] == -1)                  # beyond count, every word
    assert np.array_equal(host(E.coco_match_batch(*args)), first)                              # a second run, its own buffer
    if limits == "coco" and max_obj == 70:                                                     # every value occurs
        values = np.unique(CE.match_values(first[np.arange(max_out)[None, :] < count[:, None]], 10))
        assert set(values.tolist()) == {0, 1, 2}


@gpu
def test_hand_worked_segments_on_the_device():
    from tensorflow_yolo2_amd import engine as E
    for case in K.HAND:
        for row_form in (0, 1):
            rows, gt, area, crowd, thresholds, ranges, expect = K.hand_case(case, row_form)
            m = max(len(gt), 1)
            boxes, ar, cr = np.zeros((1, m, 5)), np.zeros((1, m)), np.zeros((1, m), np.uint8)
            boxes[0, :len(gt)], ar[0, :len(gt)], cr[0, :len(gt)] = gt, area, crowd
            got = E.coco_match_batch(dev(rows[None]), dev(np.array([len(rows)], np.int32)), dev(boxes), dev(ar), dev(cr),
                                     dev(np.array([len(gt)], np.int32)), None, thresholds, ranges, row_form)
            assert np.array_equal(host(got)[0], expect), (case[0], row_form)


@gpu
def test_bad_arguments_launch_nothing():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    out = torch.full((64,), 12345, dtype=torch.int32, device="cuda")
    p, o = C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr())

    def call(det=p, count=p, boxes=p, area=p, crowd=p, counts=p, index=p, n=1, max_obj=2, max_out=2, thr=p, T=10, rng=p,
             A=4, row_form=0, match=o):
        return lib.y2_coco_match_batch(det, count, boxes, area, crowd, counts, index, n, max_obj, max_out, thr, T, rng, A,
                                       row_form, match, None)

    for bad, text in ((dict(det=None), b"null"), (dict(count=None), b"null"), (dict(boxes=None), b"null"),
                      (dict(area=None), b"null"), (dict(crowd=None), b"null"), (dict(counts=None), b"null"),
                      (dict(thr=None), b"null"), (dict(rng=None), b"null"), (dict(match=None), b"null"),
                      (dict(T=17), b"T = 17"), (dict(T=0), b"T = 0"), (dict(A=5), b"A = 5"), (dict(A=0), b"A = 0"),
                      (dict(row_form=2), b"row_form = 2"), (dict(row_form=-1), b"row_form = -1"),
                      (dict(max_obj=257), b"max_obj = 257"), (dict(max_obj=0), b"max_obj = 0"),
                      (dict(max_out=0), b"max_out = 0"), (dict(max_out=65537), b"max_out = 65537"),
                      (dict(n=0), b"n = 0"), (dict(n=65535 * 80 + 1), b"n = 5242801")):
        assert call(**bad) == -1, bad
        err = lib.y2_last_error()
        assert b"y2_coco_match_batch" in err and text in err, (bad, err)
    torch.cuda.synchronize()
    assert bool((out == 12345).all())                         # nothing was written
    assert call(index=None) == 0                              # index may be NULL: zero counts, the -1s alone
    torch.cuda.synchronize()
    assert host(out)[:8].tolist() == [-1] * 8 and host(out)[8] == 12345


@gpu
def test_engine_contract():
    import torch
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(5)
    tabs = tables(5, 0, rng)
    det, count, index = segments(tabs[0], tabs[3], 8, 0, rng, mixed=False)
    good = dict(det=dev(det), count=dev(count), boxes=dev(tabs[0]), area=dev(tabs[1]), crowd=dev(tabs[2]),
                counts=dev(tabs[3]), index=dev(index))
    out = torch.full((12, 8, 4), 777, dtype=torch.int32, device="cuda")
    assert E.coco_match_batch(out=out, **good) is out
    want = host(out)
    assert np.array_equal(want, expected(det, count, index, tabs, None, None, 0))
    assert np.array_equal(host(E.coco_match_batch(out=out.view(-1), **good)).reshape(12, 8, 4), want)   # a view of the count
    # thresholds / area ranges as device tensors
    thr, rngs = dev(np.array([0.5, 0.75])), dev(np.array([[0.0, 1e10]]))
    assert np.array_equal(host(E.coco_match_batch(thresholds=thr, area_ranges=rngs, **good)),
                          expected(det, count, index, tabs, [0.5, 0.75], [[0, 1e10]], 0))
    # a malformed tensor raises before the launch: the output keeps its fill
    out.fill_(777)
    for name, bad in (("det", good["det"].to(torch.int64)), ("det", good["det"][:, :, :5]), ("count", good["count"][:5]),
                      ("boxes", good["boxes"].float()), ("boxes", good["boxes"].cpu()), ("area", good["area"][:, :4]),
                      ("crowd", good["crowd"].to(torch.int32)), ("counts", good["counts"][:2]),
                      ("index", good["index"].to(torch.int64)), ("index", good["index"][:11]),
                      ("area", good["area"].t().contiguous().t())):
        with pytest.raises(AssertionError):
            E.coco_match_batch(out=out, **dict(good, **{name: bad}))
    with pytest.raises(AssertionError):
        E.coco_match_batch(out=torch.empty((12, 8, 3), dtype=torch.int32, device="cuda"), **good)
    with pytest.raises(AssertionError):
        E.coco_match_batch(thresholds=dev(np.array([0.5], np.float32)), out=out, **good)
    with pytest.raises(ValueError, match="row_form 2 is neither 0"):
        E.coco_match_batch(row_form=2, out=out, **good)
    with pytest.raises(ValueError, match="17 thresholds and 4 area ranges: at most 16 and 4"):
        E.coco_match_batch(thresholds=np.linspace(0.1, 0.9, 17), out=out, **good)
    with pytest.raises(ValueError, match="max_obj = 257: the matcher holds at most 256"):
        E.coco_match_batch(good["det"], good["count"], dev(np.zeros((3, 257, 5))), dev(np.zeros((3, 257))),
                           dev(np.zeros((3, 257), np.uint8)), good["counts"], good["index"], out=out)
    torch.cuda.synchronize()
    assert bool((out == 777).all())


# ---------------------------------------------------------------- the ground truths as their own detections
TEACHER = [(3, [(10, 10, 100, 100, 0, 10000, 0), (200, 40, 30, 20, 0, 600, 0), (150, 200, 60, 50, 1, 2900, 0),
                (0, 0, 300, 300, 1, 70000, 1)]),
           (1, [(5, 5, 40, 40, 0, 1500, 0), (5, 5, 40, 40, 2, 1600, 0)]),
           (2, [])]


@gpu
@pytest.mark.parametrize("row_form", [0, 1])
def test_ground_truths_as_rows_score_one(row_form):
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.img_dataset import device_coco
    ds = K.make_dataset(TEACHER)
    tabs = device_coco.build_tables(ds["images"])
    assert tabs[0].shape == (3, 4, 5) and tabs[3].tolist() == [2, 0, 4]              # ascending image id: 1, 2, 3
    ncls, R_ = 3, 4
    det = np.full((3 * ncls, R_, 6), -1, np.int32)
    count = np.zeros(3 * ncls, np.int32)
    score = np.zeros((3 * ncls, R_), np.float32)
    for e, im in enumerate(ds["images"]):
        for c in range(ncls):
            boxes = [o["bbox"] for o in im["anns"] if o["category"] == c]
            s = e * ncls + c
            count[s] = len(boxes)
            det[s, :len(boxes)] = K.rows_from_xywh(np.reshape(boxes, (-1, 4)), [c] * len(boxes), row_form)
            score[s, :len(boxes)] = np.linspace(0.9, 0.5, len(boxes))
    index = np.repeat(np.arange(3), ncls).astype(np.int32)
    match = host(E.coco_match_batch(dev(det), dev(count), *[dev(t) for t in tabs], dev(index), row_form=row_form))
    live = np.arange(R_)[None, :] < count[:, None]
    rows = {"image": np.nonzero(live)[0] // ncls, "class": det[live][:, 4], "score": score[live], "match": match[live]}
    assert np.array_equal(rows["match"], K.rematch(rows, ds, det[live], row_form))
    stats = CE.summarize(*CE.accumulate(rows, ds))
    assert all(abs(stats[i] - 1.0) < 1e-12 for i in (0, 1, 2, 3, 4, 5, 8))           # AP of every kind, AR100
    assert rows["match"][-1].tolist() == [K.ALL_IG] * 4                              # the crowd region's own box


# ---------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def model(tmp_path_factory, golden_dir):
    from tensorflow_yolo2_amd.utils import darknet_cfg, darknet_weights as DW
    cfg = os.path.join(golden_dir, "cfg", "narrow-tiny-coco.cfg")
    rec = darknet_cfg.load(cfg)
    path = str(tmp_path_factory.mktemp("coco") / "narrow-tiny-coco.weights")
    DW.write(path, R.random_layers(rec.file_layers, 80), 64000)
    return cfg, path


@gpu
@pytest.mark.parametrize("protocol", ["repo", "letterbox", "darknet"])
def test_coco_eval_end_to_end(model, golden_dir, tmp_path, capsys, protocol):
    from tensorflow_yolo2_amd.coco import coco_eval_yolov2
    cfg, weights = model
    results = str(tmp_path / "results.json")
    argv = ["--annotations", os.path.join(golden_dir, "coco", "instances_tiny.json"), "--images", golden_dir, "--cfg", cfg,
            "--darknet-weights", weights, "--batch", "2", "--thresh", "0.02", "--max-per-class", "8", "--results", results]
    argv += {"repo": [], "letterbox": ["--letterbox"], "darknet": ["--protocol", "darknet"]}[protocol]
    res = coco_eval_yolov2.main(argv)
    printed = capsys.readouterr().out
    rows, ds, row_form = res["rows"], res["imdb"].dataset, 1 if protocol == "darknet" else 0
    assert len(rows["score"]) > 9 and res["count"].shape == (3, 3) and res["count"].sum() == len(rows["score"])
    assert [e["id"] for e in res["imdb"].entries] == [7, 19, 42] and res["imdb"].category_ids == [1, 3, 17]
    assert rows["box"].dtype == (np.float32 if row_form else np.int32)
    raw = np.concatenate([np.ascontiguousarray(rows["box"]).view(np.int32), rows["class"][:, None],
                          rows["candidate"][:, None]], axis=1)
    assert np.array_equal(rows["match"], K.rematch(rows, ds, raw, row_form))         # the device's words are the spec's
    stats = CE.summarize(*CE.accumulate(dict(rows, match=K.rematch(rows, ds, raw, row_form)), ds))
    assert res["stats"] == stats and len(stats) == 12
    for line in CE.summary_lines(stats):
        assert line in printed
    back = json.load(open(results))
    assert len(back) == len(rows["score"]) and set(r["category_id"] for r in back) <= {1, 3, 17}
    assert set(r["image_id"] for r in back) <= {7, 19, 42}
    assert [r["category_id"] for r in back] == [ds["categories"][c] for c in rows["class"]]
    assert np.allclose([r["bbox"] for r in back], rows["bbox"], atol=1e-6)


@gpu
def test_coco_eval_argument_errors(model, golden_dir, tmp_path, capsys):
    from tensorflow_yolo2_amd.coco import coco_eval_yolov2
    cfg, weights = model
    base = ["--annotations", os.path.join(golden_dir, "coco", "instances_tiny.json"), "--images", golden_dir, "--batch", "2"]
    with pytest.raises(SystemExit):
        coco_eval_yolov2.main(base + ["--cfg", os.path.join(golden_dir, "cfg", "narrow-tiny-voc.cfg")])
    assert "20 classes" in capsys.readouterr().err
    names = tmp_path / "two.names"
    names.write_text("person\ncar\n")
    with pytest.raises(SystemExit):
        coco_eval_yolov2.main(base + ["--cfg", cfg, "--darknet-weights", weights, "--names", str(names)])
    assert "holds 2 names, the model has 3 classes" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        coco_eval_yolov2.main(["--annotations", str(tmp_path / "none.json"), "--images", golden_dir, "--cfg", cfg])
    assert "none.json" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        coco_eval_yolov2.main(base + ["--cfg", cfg, "--protocol", "darknet", "--fill", "3"])
    assert "--fill is not read" in capsys.readouterr().err
