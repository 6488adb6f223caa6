"""Evaluation on the device: y2_detect_grid_batch and y2_voc_match_batch (csrc/detect.hip) bit for bit against
utils/detect_batch.py, DeviceVOC.eval_batch, and pascal_eval_darknet.main against the host composition of the same
forward outputs.  Everything here is equality: no tolerance anywhere.  The first test needs no GPU: it checks that the
specification alone exercises every rule on the inputs the GPU tests use."""
import ctypes as C
import os

import numpy as np
import pytest

from test_device_voc_host import make_devkit
from tensorflow_yolo2_amd.utils import detect_batch as DB

gpu = pytest.mark.gpu

NUM_CLASS, B = 20, 2
D = NUM_CLASS + 5 * B
SHAPES = ((333, 500), (500, 375), (240, 352), (97, 150))      # (height, width) of the hand-made table's entries
OBJECT_THRESH, IOU_THRESH, MAX_OUT = 0.2, 0.45, 24


def _table():
    return np.array([(0, h, w, 16 * ((3 * w + 15) // 16), 0) for (h, w) in SHAPES], np.int64)


def _put(p, S, cell, b, conf=None, box=None, cls=None):
    row = p.reshape(S * S, D)[cell]
    if conf is not None:
        row[NUM_CLASS + b] = conf
    if box is not None:
        row[NUM_CLASS + B + 4 * b:NUM_CLASS + B + 4 * b + 4] = box
    if cls is not None:
        row[:NUM_CLASS] = 0.1
        row[cls] = 0.9


def _detect_case(S):
    """(predict [3][S][S][30], {name: candidate index in image 0}).  Image 0 holds the hand-made candidates, image 1 has
    nothing above the threshold, image 2 has small boxes with high confidences: more survivors than MAX_OUT."""
    rng = np.random.default_rng(1000 + S)
    p = rng.uniform(0.0, 1.0, (3, S, S, D)).astype(np.float32)
    p[..., NUM_CLASS + B:] = rng.uniform(0.0, 0.75, (3, S, S, 4 * B))
    p[..., NUM_CLASS:NUM_CLASS + B] = rng.uniform(0.0, 0.6, (3, S, S, B))
    p[1, ..., NUM_CLASS:NUM_CLASS + B] *= 0.3                             # image 1: every confidence below 0.2
    p[1, 0, 0, NUM_CLASS] = OBJECT_THRESH                                 # equal to the threshold is not above it
    p[2, ..., NUM_CLASS:NUM_CLASS + B] = rng.uniform(0.5, 1.0, (S, S, B))
    p[2, ..., NUM_CLASS + B + 2::4] = rng.uniform(0.1, 0.2, (S, S, B))
    p[2, ..., NUM_CLASS + B + 3::4] = rng.uniform(0.1, 0.2, (S, S, B))
    q, named = p[0], {}

    def put(name, cell, b, **kw):
        _put(q, S, cell, b, **kw)
        named[name] = cell * B + b
    mid = (S // 2) * S + S // 2
    box = (0.5, 0.5, 0.3, 0.3)
    put("twin_a", mid, 0, conf=0.99, box=box, cls=3)                      # one cell, two predictors, the same box
    put("twin_b", mid, 1, conf=0.98, box=box)
    put("shift_a", mid + S, 0, conf=0.97, box=box, cls=4)                 # identical pixels from the neighbouring cell
    put("shift_same", mid + S + 1, 0, conf=0.96, box=(-0.5, 0.5, 0.3, 0.3), cls=4)    # ... in the same class
    put("shift_other", mid + S - 1, 0, conf=0.95, box=(1.5, 0.5, 0.3, 0.3), cls=5)    # ... and in another class
    put("nan_conf", 0, 0, conf=np.nan, box=box)
    put("inf_field", 1, 0, conf=0.94, box=(np.inf, 0.5, 0.3, 0.3))
    put("huge_field", 2, 0, conf=0.94, box=(0.5, 0.5, 0.3, 1e10))         # 1e20 * height
    put("zero_width", 3, 0, conf=0.94, box=(0.5, 0.5, 0.0, 0.3))
    put("outside", 4, 0, conf=0.94, box=(50.0, 0.5, 0.2, 0.2), cls=6)
    put("partly_outside", S - 1, 0, conf=0.93, box=(0.9, 0.1, 0.6, 0.6), cls=7)
    put("larger_than_image", mid - S, 0, conf=0.92, box=(0.5, 0.5, 1.2, 1.3), cls=8)
    for k in range(6):                                                    # a run of equal confidences, two classes
        put("run%d" % k, (S - 2) * S + k, 1, conf=0.5, box=(0.5, 0.5, 0.12, 0.12))
        _put(q, S, (S - 2) * S + k, 0, conf=0.1, cls=9 + k % 2)
    return p, named


def _spec_detect(p, entries, object_thresh, iou_thresh, max_out):
    out = []
    for k, e in enumerate(entries):
        h, w = SHAPES[e]
        out.append(DB.grid_detect(p[k], w, h, NUM_CLASS, B, object_thresh, iou_thresh, max_out))
    return out


@pytest.mark.parametrize("S", (7, 13, 19))
def test_detect_inputs_exercise_every_rule(S):
    """no GPU: on these inputs the specification alone suppresses, cuts, drops for every reason, runs out of max_out
    and meets equal scores -- otherwise the bit-equality below would show nothing"""
    p, named = _detect_case(S)
    K = S * S * B
    assert K not in (64, 128, 256, 512, 1024)
    h, w = SHAPES[0]
    valid, box, cls, score = DB.grid_candidates(p[0], w, h, NUM_CLASS, B, OBJECT_THRESH)
    for name in ("nan_conf", "inf_field", "huge_field", "zero_width", "outside"):
        assert not valid[named[name]], name
        assert name == "nan_conf" or score[named[name]] > OBJECT_THRESH
    for name in ("twin_a", "twin_b", "shift_a", "shift_same", "shift_other", "partly_outside", "larger_than_image"):
        assert valid[named[name]], name
    assert box[named["twin_a"]].tolist() == box[named["twin_b"]].tolist()
    assert box[named["shift_a"]].tolist() == box[named["shift_same"]].tolist() == box[named["shift_other"]].tolist()
    assert box[named["larger_than_image"]].tolist() == [1, 1, w, h]
    assert box[named["partly_outside"]][2] == w and box[named["partly_outside"]][1] == 1
    full, _ = DB.grid_detect(p[0], w, h, NUM_CLASS, B, OBJECT_THRESH, IOU_THRESH, K)
    kept = set(full[:, 5].tolist())
    assert len(kept) < valid.sum()                                        # something is suppressed
    assert named["twin_a"] in kept and named["twin_b"] not in kept
    assert named["shift_a"] in kept and named["shift_same"] not in kept and named["shift_other"] in kept
    runs = [named["run%d" % k] for k in range(6)]
    assert sorted(i for i in full[:, 5].tolist() if i in runs) == [i for i in full[:, 5].tolist() if i in runs] != []
    (d0, _s0), (d1, _s1), (d2, _s2) = _spec_detect(p, (0, 1, 2), OBJECT_THRESH, IOU_THRESH, MAX_OUT)
    assert len(d1) == 0 and len(d2) == MAX_OUT
    assert len(DB.grid_detect(p[2], SHAPES[2][1], SHAPES[2][0], NUM_CLASS, B, OBJECT_THRESH, IOU_THRESH, K)[0]) > MAX_OUT
    none, _ = DB.grid_detect(p[0], w, h, NUM_CLASS, B, OBJECT_THRESH, 1.0, K)
    assert len(none) == valid.sum() and {named["twin_b"], named["shift_same"]} <= set(none[:, 5].tolist())
    every, _ = DB.grid_detect(p[0], w, h, NUM_CLASS, B, OBJECT_THRESH, 0.0, K)
    assert len(every) < len(full)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_detect(p, entries, index, object_thresh, iou_thresh, max_out):
    import torch
    from tensorflow_yolo2_amd import engine as E
    table = torch.from_numpy(_table()).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
    n = len(entries)
    out = (torch.full((n, max_out, 6), 77, dtype=torch.int32, device="cuda"),
           torch.full((n, max_out), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    det, score, count = E.detect_grid_batch(torch.from_numpy(p).cuda(), table, idx, NUM_CLASS, B, object_thresh,
                                            iou_thresh, max_out, out=out)
    torch.cuda.synchronize()
    det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    for k, (want_det, want_score) in enumerate(_spec_detect(p, entries, object_thresh, iou_thresh, max_out)):
        c = len(want_det)
        assert count[k] == c, (k, count[k], c)
        assert np.array_equal(det[k, :c], want_det), k
        assert np.array_equal(score[k, :c].view(np.uint32), want_score.view(np.uint32)), k
        assert (det[k, c:] == -1).all() and (score[k, c:] == 0).all()
    return count


@gpu
@pytest.mark.parametrize("S", (7, 13, 19))
def test_detect_is_bit_equal_to_the_specification(S):
    p, _named = _detect_case(S)
    K = S * S * B
    count = _check_detect(p, (0, 1, 2), None, OBJECT_THRESH, IOU_THRESH, MAX_OUT)
    assert count.tolist()[1:] == [0, MAX_OUT] and 0 < count[0] <= MAX_OUT
    _check_detect(p, (3, 1, 1), (3, 1, 1), OBJECT_THRESH, IOU_THRESH, MAX_OUT)     # through an index, other sizes
    _check_detect(p, (0, 1, 2), None, OBJECT_THRESH, IOU_THRESH, K)                # nothing cut off by max_out
    _check_detect(p, (0, 1, 2), (0, 1, 2), OBJECT_THRESH, 1.0, K)                  # nothing suppressed
    _check_detect(p, (2, 0, 3), (2, 0, 3), OBJECT_THRESH, 0.0, K)                  # every overlap suppressed
    _check_detect(p, (0, 1, 2), None, -1.0, IOU_THRESH, K)                         # every confidence passes


def _match_case(max_obj, seed):
    """(det [n][max_out][6], count [n], boxes [E][max_obj][5], counts [E], difficult [E][max_obj]), E = n"""
    rng = np.random.default_rng(seed)
    n, max_out = 8, 40
    boxes = np.zeros((n, max_obj, 5))
    counts = np.zeros(n, np.int32)
    difficult = np.zeros((n, max_obj), np.uint8)
    det = np.full((n, max_out, 6), -1, np.int32)
    count = np.zeros(n, np.int32)
    for k in range(n):
        m = (max_obj, 0, 1)[k] if k < 3 else int(rng.integers(1, max_obj + 1))
        counts[k] = m
        for j in range(m):
            x, y = rng.integers(1, 300, 2)
            boxes[k, j] = (x, y, x + rng.integers(8, 100), y + rng.integers(8, 100), rng.integers(0, 3))
        boxes[k, m:] = (1, 1, 400, 400, 0)                                # beyond the count: never read
        difficult[k, :m] = rng.random(m) < 0.3
        difficult[k, m:] = 1
        c = (max_out, 12, 12, 0)[k] if k < 4 else int(rng.integers(1, max_out + 1))
        count[k] = c
        for d in range(c):
            if m and rng.random() < 0.75:
                g = boxes[k, rng.integers(0, m)]
                jit = rng.integers(-5, 6, 4) * (rng.random() < 0.6)       # 40 %: exactly on the object (duplicates)
                det[k, d, :5] = np.concatenate([g[:4] + jit, [g[4] if rng.random() < 0.9 else 3]])
            else:
                x, y = rng.integers(1, 300, 2)
                det[k, d, :5] = (x, y, x + rng.integers(8, 100), y + rng.integers(8, 100), rng.integers(0, 4))
            det[k, d, 5] = d
    # image 0 by hand: an IoU tie between two objects (the first wins, then the detection's twin meets it taken), IoU
    # exactly at the threshold, just below it, a difficult object, a class without objects
    boxes[0, :3] = [(10, 10, 59, 59, 1), (40, 10, 89, 59, 1), (101, 1, 110, 10, 2)]
    difficult[0, :3] = (0, 0, 0)
    boxes[0, 3:counts[0], 4] = 0
    det[0, :6, :5] = [(25, 10, 74, 59, 1), (25, 10, 74, 59, 1), (25, 10, 74, 59, 1), (101, 1, 110, 20, 2),
                      (101, 1, 110, 21, 2), (10, 10, 59, 59, 3)]
    if max_obj > 64:                  # the same object in two strides of one lane, and in two lanes of the second stride
        boxes[0, 2 + 64] = boxes[0, 2]
        boxes[0, 66 + 1], boxes[0, 69] = (200, 200, 240, 260, 2), (200, 200, 240, 260, 2)
        difficult[0, 66], difficult[0, 67], difficult[0, 69] = 1, 0, 1
        det[0, 6:9, :5] = [(200, 200, 240, 260, 2), (200, 200, 240, 260, 2), (101, 1, 110, 10, 2)]
    return det, count, boxes, counts, difficult


def _spec_match(det, count, boxes, counts, difficult, entries, iou_thresh):
    want = np.full(det.shape[:2], -1, np.int32)
    for k, e in enumerate(entries):
        want[k, :count[k]] = DB.match_image(det[k, :count[k]], boxes[e, :counts[e]], difficult[e, :counts[e]], iou_thresh)
    return want


@gpu
@pytest.mark.parametrize("max_obj", (3, 70))
def test_match_is_bit_equal_to_the_specification(max_obj):
    import torch
    from tensorflow_yolo2_amd import engine as E
    det, count, boxes, counts, difficult = _match_case(max_obj, 50 + max_obj)
    n = len(det)
    want = _spec_match(det, count, boxes, counts, difficult, range(n), 0.5)
    # the case holds what it is meant to hold (specification alone)
    assert want[0, :6].tolist() == [1, 0, 0, 1, 0, 0]
    if max_obj > 64:
        assert want[0, 6:9].tolist() == [1, 0, 0]        # object 67 (not difficult) before 69; then taken; 2 before 66
    assert (want == 2).sum() > 5 and (want == 1).sum() > 5 and (want == 0).sum() > 10 and (want[3] == -1).all()
    dev = [torch.from_numpy(a).cuda() for a in (det, count, boxes, counts, difficult)]
    got = E.voc_match_batch(dev[0], None, dev[1], dev[2], dev[3], dev[4], None, 0.5)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    # through an index: the detections of slot k against the objects of another entry
    index = [(k + 3) % n for k in range(n)]
    want = _spec_match(det, count, boxes, counts, difficult, index, 0.5)
    got = E.voc_match_batch(dev[0], None, dev[1], dev[2], dev[3], dev[4],
                            torch.tensor(index, dtype=torch.int32, device="cuda"), 0.5)
    assert np.array_equal(got.cpu().numpy(), want)


@gpu
def test_detect_and_match_argument_errors():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    for (n, S, b, max_out) in ((1, 23, 2, 10), (1, 19, 3, 10), (0, 7, 2, 10), (1, 7, 2, 0)):
        assert lib.y2_detect_grid_batch(p, p, None, n, S, b, 20, 0.1, 0.5, max_out, p, p, p, None) == -1
        assert b"y2_detect_grid_batch" in lib.y2_last_error()
    assert b"max_out" in lib.y2_last_error()
    for (n, max_obj, max_out) in ((1, 1025, 10), (1, 0, 10), (0, 3, 10), (1, 3, 0)):
        assert lib.y2_voc_match_batch(p, None, p, p, p, p, None, n, max_obj, max_out, 0.5, p, None) == -1
        assert b"y2_voc_match_batch" in lib.y2_last_error()
    assert lib.y2_voc_match_batch(None, None, p, p, p, p, None, 1, 3, 10, 0.5, p, None) == -1
    torch.cuda.synchronize()


@gpu
def test_eval_batch_walks_the_list_and_leaves_the_cursor(tmp_path, golden_dir):
    import torch
    from oracle import data_ref as R
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import imread_bgr
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)          # 3 images
    plain = DeviceVOC("trainval", batch_size=2, devkit_path=kit, flipped=False, seed=3)
    seq = [tuple(t.cpu().numpy().copy() for t in plain.get(64)) for _ in range(4)]
    ds = DeviceVOC("trainval", batch_size=2, devkit_path=kit, flipped=False, seed=3)
    got = [tuple(t.cpu().numpy().copy() for t in ds.get(64))]
    want = [R.resize_bilinear_u8(imread_bgr(e["imname"]), 96, 96) for e in ds.entries]
    for start, slots, valid in ((0, (0, 1), 2), (2, (2, 2), 1)):              # the last batch repeats its final entry
        images, nvalid = ds.eval_batch(96, start)
        torch.cuda.synchronize()
        assert nvalid == valid and ds.eval_index.cpu().tolist() == list(slots)
        assert np.array_equal(images.cpu().numpy(), np.stack([want[s] for s in slots]))
    got += [tuple(t.cpu().numpy().copy() for t in ds.get(64)) for _ in range(3)]
    for a, b in zip(seq, got):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert ds.difficult.cpu().numpy().tolist() == [[0] * ds.max_obj] * 2 + [[0, 0, 1] + [0] * (ds.max_obj - 3)]
    with pytest.raises(IndexError):
        ds.eval_batch(96, 3)
    flipped = DeviceVOC("trainval", batch_size=2, devkit_path=kit, flipped=True, seed=3)
    with pytest.raises(ValueError, match="flipped"):
        flipped.eval_batch(96, 0)


@gpu
def test_eval_script_equals_the_host_composition(tmp_path, golden_dir, capsys):
    """3 images in batches of 2 (one partial batch) on the initial values: rows, flags and APs are those of grid_detect,
    match_image and map_from_flags on the SAME forward outputs.  On the moving statistics the initial values (filters of
    standard deviation 0.1, 22 layers) grow the activations until every decoded product is beyond 2^30 and nothing is
    detected; with --head-batch-stats the head's outputs are of order 1, so confidences, classes and boxes vary from cell
    to cell and detections exist."""
    from tensorflow_yolo2_amd.pascal import pascal_eval_darknet
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import CLASSES
    from tensorflow_yolo2_amd.yolo2_nets import darknet
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    argv = ["--devkit", kit, "--image-set", "trainval", "--size", "224", "--batch", "2", "--dtype", "f32",
            "--thresh", "0.0", "--nms", "0.45", "--max-out", "30", "--metric", "10", "--keep-predicts",
            "--head-batch-stats"]
    darknet.reset_default_graph()
    try:
        r = pascal_eval_darknet.main(argv)
        predicts = r["predicts"].cpu().numpy()
        entries = r["imdb"].entries
    finally:
        darknet.reset_default_graph()
        darknet.set_default_dtype("f16")
    assert predicts.shape == (3, 7, 7, 30) and np.isfinite(predicts).all()
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    for k, e in enumerate(entries):
        det, score = DB.grid_detect(predicts[k], e["shape"][1], e["shape"][0], 20, 2, 0.0, 0.45, 30)
        flag = DB.match_image(det, np.asarray(e["objs"], np.float64), e["difficult"], 0.5)
        rows["image"] += [k] * len(det)
        rows["box"] += det[:, :4].tolist()
        rows["class"] += det[:, 4].tolist()
        rows["candidate"] += det[:, 5].tolist()
        rows["score"] += score.tolist()
        rows["flag"] += flag.tolist()
    assert len(rows["image"]) > 20 and set(rows["image"]) == {0, 1, 2}       # detections exist in every image
    for key in rows:
        assert r["rows"][key].tolist() == rows[key], key
    npos = DB.npos_from_objects([o[4] for e in entries for o in e["objs"]], [d for e in entries for d in e["difficult"]])
    assert r["npos"] == npos and npos[CLASSES.index("bird")] == 0            # the only bird is difficult: AP 0, counted
    want = DB.map_from_flags((np.array(rows["class"]), np.array(rows["score"], np.float32), np.array(rows["flag"])),
                             npos, use_07_metric=False)
    assert (r["mAP"], r["aps"]) == want and sorted(r["aps"]) == sorted(npos)
    out = capsys.readouterr().out
    assert "Mean AP = %.4f" % want[0] in out and "AP for bird = 0.0000" in out
