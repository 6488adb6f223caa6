"""One detection row per (candidate, class) from the device pool: y2_detect_anchor_classes_batch (csrc/detect.hip) bit
for bit against utils/detect_batch.anchor_detect_classes fed with the device's own y2_decode_anchors, y2_voc_match_batch
over the (image, class) segments against match_image per segment, and pascal_eval_yolov2 --per-class against the host
composition on the same head outputs.  Everything is equality: no tolerance.  tests/test_anchor_classes_host.py checks
without a GPU that these inputs hold what per-class rows add."""
import ctypes as C
import os

import numpy as np
import pytest

from test_anchor_classes_host import HAND_CAND, HAND_GT, HAND_H, HAND_W, _relative
from test_device_voc_host import make_devkit
from test_gpu_detect_anchor import ANCHORS, GEOMETRIES, SHAPES, _anchor_case, _host_rows, _table, _unit_gain_layers
from tensorflow_yolo2_amd.utils import detect_batch as DB

gpu = pytest.mark.gpu

IOU_THRESH, MAX_PER_CLASS = 0.45, 8
MIXED_THRESH = 3e-4      # (19, 5, 20): image 1's segments hold a handful of candidates, image 0's more than 1024


def _launch(dev, B, index, score_thresh, max_per_class):
    """(det, score, count) as numpy, written over sentinels"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    n, ncls = dev.shape[0], dev.shape[4] - 5
    table = torch.from_numpy(_table()).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
    out = (torch.full((n, ncls, max_per_class, 6), 77, dtype=torch.int32, device="cuda"),
           torch.full((n, ncls, max_per_class), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((n, ncls), 77, dtype=torch.int32, device="cuda"))
    got = E.detect_anchor_classes_batch(dev, ANCHORS[:B], table, idx, score_thresh, IOU_THRESH, max_per_class, out=out)
    torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in got)


def _check(dev, decoded, B, entries, index, score_thresh, max_per_class):
    boxes, scores = decoded
    det, score, count = _launch(dev, B, index, score_thresh, max_per_class)
    for k, e in enumerate(entries):
        want = DB.anchor_detect_classes(boxes[k], scores[k], SHAPES[e][1], SHAPES[e][0], score_thresh, IOU_THRESH,
                                        max_per_class)
        assert np.array_equal(count[k], want[2]), (k, count[k], want[2])
        assert np.array_equal(det[k], want[0]), k                         # unused rows are -1 in both
        assert np.array_equal(score[k].view(np.uint32), want[1].view(np.uint32)), k
    return count


@gpu
@pytest.mark.parametrize("S,B,C", GEOMETRIES)
def test_detect_anchor_classes_is_bit_equal_to_the_specification(S, B, C):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    dev = torch.from_numpy(net).cuda()
    boxes, scores = E.decode_anchors(dev, ANCHORS[:B])
    decoded = (boxes.cpu().numpy(), scores.cpu().numpy())
    for thresh in (0.02, 0.005):
        count = _check(dev, decoded, B, (0, 1, 2), None, thresh, MAX_PER_CLASS)
        if S > 1:
            assert (count[0] == MAX_PER_CLASS).all() and (count[1] == 0).all() and (count[2] == MAX_PER_CLASS).all()
        full = _check(dev, decoded, B, (2, 0, 3), (2, 0, 3), thresh, K)   # an index, other sizes, nothing capped
        assert S == 1 or (full[0] > MAX_PER_CLASS).all()                  # (image 0's head at entry 2's size)
    # the compacted sort at its smallest and its largest width in one launch
    valid = np.array([[DB.anchor_candidates(decoded[0][k], decoded[1][k][:, c], np.full(K, c), SHAPES[k][1],
                                            SHAPES[k][0], MIXED_THRESH)[0].sum() for c in range(C)] for k in range(3)])
    if (S, B, C) == (19, 5, 20):
        assert 0 < valid[1].max() < 64 and valid[0].min() > 1024 and 64 < valid[2].min() and valid[2].max() <= 1024
    _check(dev, decoded, B, (0, 1, 2), None, MIXED_THRESH, MAX_PER_CLASS)
    _check(dev, decoded, B, (0, 1, 2), (0, 1, 2), MIXED_THRESH, K)


@gpu
def test_two_launches_give_identical_bytes():
    import torch
    S, B, ncls = 19, 5, 20
    dev = torch.from_numpy(_anchor_case(S, B, ncls)[0]).cuda()
    for thresh in (0.005, MIXED_THRESH):
        first = _launch(dev, B, (2, 0, 3), thresh, MAX_PER_CLASS)
        second = _launch(dev, B, (2, 0, 3), thresh, MAX_PER_CLASS)
        for a, b in zip(first, second):
            assert a.tobytes() == b.tobytes()
        assert first[2].max() == MAX_PER_CLASS


@gpu
def test_match_over_segments_equals_match_image_per_segment():
    """the hand-made images of the host test (a difficult object, two detections on one object, a class holding two
    objects): y2_voc_match_batch over the [n * C] view, every image's entry named C times by an index made on the
    device, against match_image on each (image, class) segment"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    n, ncls, M, max_obj = len(HAND_CAND), 3, 4, 4
    det = np.empty((n, ncls, M, 6), np.int32)
    score = np.empty((n, ncls, M), np.float32)
    count = np.empty((n, ncls), np.int32)
    gt = np.zeros((n, max_obj, 5))
    gt_count = np.zeros(n, np.int32)
    difficult = np.ones((n, max_obj), np.uint8)
    want = np.full((n, ncls, M), -1, np.int32)
    for k in range(n):
        boxes = np.array([_relative(b, HAND_W, HAND_H) for b, _s in HAND_CAND[k]], np.float32)
        sc = np.array([s for _b, s in HAND_CAND[k]], np.float32)
        det[k], score[k], count[k] = DB.anchor_detect_classes(boxes, sc, HAND_W, HAND_H, 0.1, IOU_THRESH, M)
        m = gt_count[k] = len(HAND_GT[k])
        gt[k, :m] = [b + (c,) for b, c, _d in HAND_GT[k]]
        difficult[k, :m] = [d for _b, _c, d in HAND_GT[k]]
        for c in range(ncls):
            want[k, c, :count[k, c]] = DB.match_image(det[k, c, :count[k, c]], gt[k, :m], difficult[k, :m], 0.5)
    assert {0, 1, 2} <= set(want.ravel().tolist()) and want[0, 0].tolist() == [1, 0, 0, -1]
    for entries in ((0, 1, 2), (2, 0, 1)):                                 # the pool's order, and through an index
        e = list(entries)
        dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (det[e], score[e], count[e])]
        pool = [torch.from_numpy(a).cuda() for a in (gt, gt_count, difficult)]
        index = torch.tensor(e, dtype=torch.int32, device="cuda")
        seg_index = index[:, None].expand(n, ncls).contiguous().view(-1)
        flags = E.voc_match_batch(dev[0].view(n * ncls, M, 6), dev[1].view(n * ncls, M), dev[2].view(-1), pool[0],
                                  pool[1], pool[2], seg_index, 0.5)
        assert np.array_equal(flags.cpu().numpy().reshape(n, ncls, M), want[e])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@gpu
def test_detect_anchor_classes_argument_errors():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    #           n  S   B     C  max_per_class
    for case in ((1, 13, 5, 20, 0), (1, 1, 2049, 20, 10), (1, 21, 5, 20, 10), (1, 13, 17, 20, 10), (1, 13, 5, 0, 10),
                 (0, 13, 5, 20, 10)):
        n, S, B, ncls, m = case
        assert lib.y2_detect_anchor_classes_batch(p, p, p, None, n, S, B, ncls, 0.1, 0.5, m, p, p, p, None) == -1, case
        assert b"y2_detect_anchor_classes_batch" in lib.y2_last_error()
        if case == (1, 13, 5, 20, 0):
            assert b"max_per_class = 0" in lib.y2_last_error()
        if case == (1, 21, 5, 20, 10):
            assert b"2205 candidates beyond Y2_DETECT_ANCHOR_MAX_CANDIDATES = 2048" in lib.y2_last_error()
        if case == (1, 13, 17, 20, 10):
            assert b"B = 17 (at most 16)" in lib.y2_last_error()
    for null in (0, 1, 2, 11, 12, 13):
        a = [p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, p, p, p, None]
        a[null] = None
        assert lib.y2_detect_anchor_classes_batch(*a) == -1 and b"null" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


def _host_class_rows(grids, anchors, entries, thresh, nms, max_per_class):
    """the host composition on the kept grids: E.decode_anchors -> anchor_detect_classes -> match_image per segment"""
    from tensorflow_yolo2_amd import engine as E
    boxes, scores = (t.cpu().numpy() for t in E.decode_anchors(grids.contiguous(), anchors))
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    counts = []
    for k, e in enumerate(entries):
        det, score, count = DB.anchor_detect_classes(boxes[k], scores[k], e["shape"][1], e["shape"][0], thresh, nms,
                                                     max_per_class)
        counts.append(count.tolist())
        for c, m in enumerate(count):
            flag = DB.match_image(det[c, :m], np.asarray(e["objs"], np.float64), e["difficult"], 0.5)
            rows["image"] += [k] * int(m)
            rows["box"] += det[c, :m, :4].tolist()
            rows["class"] += det[c, :m, 4].tolist()
            rows["candidate"] += det[c, :m, 5].tolist()
            rows["score"] += score[c, :m].tolist()
            rows["flag"] += flag.tolist()
    return rows, counts


@gpu
@pytest.mark.parametrize("size,batch,dtype", ((224, 2, "f32"), (608, 1, "f16")))
def test_eval_script_per_class_equals_the_host_composition(tmp_path, golden_dir, capsys, size, batch, dtype):
    """test_gpu_detect_anchor's end-to-end case with --per-class: rows, flags, the saturated count, APs and mAP are
    those of anchor_detect_classes, match_image per segment and map_from_flags on the SAME head outputs; the results
    files hold the rows; and without --per-class the script returns the per-anchor composition as before"""
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import CLASSES
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    model = yolov2.YOLOv2Detector(batch, size, dtype=dtype, width_div=8, seed=4)
    for net in model.networks():
        net.load_params(_unit_gain_layers(net))
    weights = str(tmp_path / "unit_gain.npz")
    net_utils.save_yolov2_variables(model, weights, iteration=7)
    del model
    M = 6
    argv = ["--devkit", kit, "--image-set", "trainval", "--size", str(size), "--batch", str(batch), "--dtype", dtype,
            "--width-div", "8", "--weights", weights, "--thresh", "0.02", "--nms", "0.45", "--max-out", "30",
            "--metric", "10", "--keep-grids"]
    results = str(tmp_path / "results")
    r = pascal_eval_yolov2.main(argv + ["--per-class", "--max-per-class", str(M), "--results-dir", results])
    S = size // 32
    assert r["restored"] == 7 and tuple(r["grids"].shape) == (3, S, S, 5, 25)
    entries = r["imdb"].entries
    rows, counts = _host_class_rows(r["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, M)
    assert len(rows["image"]) > 20 and set(rows["image"]) == {0, 1, 2}
    assert len(set(rows["class"])) > 1                                    # an image has rows in several classes
    for key in rows:
        assert r["rows"][key].tolist() == rows[key], key
    assert r["count"].tolist() == counts
    assert r["saturated"] == sum(m == M for c in counts for m in c)
    npos = DB.npos_from_objects([o[4] for e in entries for o in e["objs"]], [d for e in entries for d in e["difficult"]])
    want = DB.map_from_flags((np.array(rows["class"]), np.array(rows["score"], np.float32), np.array(rows["flag"])),
                             npos, use_07_metric=False)
    assert (r["mAP"], r["aps"]) == want and sorted(r["aps"]) == sorted(npos)
    out = capsys.readouterr().out
    assert "Mean AP = %.4f" % want[0] in out
    assert "%d of 60 (image, class) segments reached --max-per-class %d" % (r["saturated"], M) in out
    lines = 0
    for c, path in enumerate(r["results_files"]):
        assert os.path.basename(path) == "comp4_det_trainval_%s.txt" % CLASSES[c]
        with open(path) as f:
            got = [line.split() for line in f.read().splitlines()]
        sel = [k for k, v in enumerate(rows["class"]) if v == c]
        assert [g[0] for g in got] == [r["imdb"].image_index[rows["image"][k]] for k in sel]
        assert [[int(v) for v in g[2:]] for g in got] == [rows["box"][k] for k in sel]
        lines += len(got)
    assert lines == len(rows["class"]) and len(r["results_files"]) == 20
    if size != 224:
        return
    # the default is the per-anchor evaluation, unchanged
    d = pascal_eval_yolov2.main(argv)
    assert "saturated" not in d and "results_files" not in d
    anchor_rows = _host_rows(d["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30)
    for key in anchor_rows:
        assert d["rows"][key].tolist() == anchor_rows[key], key
    assert d["count"].tolist() == [anchor_rows["image"].count(k) for k in range(3)]
    want = DB.map_from_flags((np.array(anchor_rows["class"]), np.array(anchor_rows["score"], np.float32),
                              np.array(anchor_rows["flag"])), npos, use_07_metric=False)
    assert (d["mAP"], d["aps"]) == want
