"""Detection on a word-tree head from the tree's node (csrc/detect_tree.hip) on the GPU: y2_word_tree_top bit for bit
against y2_word_tree_head's top / prob, y2_detect_anchor_tree_batch against the old two launches on the rewritten rows
(contracts E1, E2 of DESIGN.md 9) and against utils/detect_batch.anchor_detect, y2_detect_anchor_tree_batch_dk against the
per-class Darknet entry (E3) and anchor_detect_tree_darknet, the argument errors, and the path up to YOLOv2Detector,
evaluate_yolov2, darknet/detector.py and pascal_detect_yolov2 on models with a wide head.  Everything about the kernels is
equality: no tolerance but the host walk's prob (rtol 2e-5, tests/test_gpu_word_tree.py's)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

import _detect_tree_cases as T
import _wide_head_cases as WH
import _word_tree_cases as WT
import _yolo9000_cases as Y
from test_device_voc_host import make_devkit
from test_gpu_detect_anchor import ANCHORS, SHAPES, _table
from tensorflow_yolo2_amd.utils import detect_batch as DB, word_tree as W

gpu = pytest.mark.gpu
GUARD = 1024
INT_MAX = 2 ** 31 - 1


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ---- 1, 2: the walk
def _top_with_guards(src, tt, thresh, obj_thresh):
    """engine.word_tree_top into sentinel-filled buffers with a guard band behind each -> (top, prob) on the host"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    rows = src.shape[0]
    top_buf = torch.full((rows + GUARD,), -77, dtype=torch.int32, device="cuda")
    prob_buf = torch.full((rows + GUARD,), -7.0, dtype=torch.float32, device="cuda")
    top, prob = E.word_tree_top(src, tt, thresh, obj_thresh, out=(top_buf[:rows], prob_buf[:rows]))
    torch.cuda.synchronize()
    assert (top_buf[rows:] == -77).all() and (prob_buf[rows:] == -7.0).all()   # nothing behind the outputs
    top, prob = top.cpu().numpy(), prob.cpu().numpy()
    assert not (top == -77).any() and not (prob == -7.0).any()                  # every word was written
    return top, prob


def _walk_input(name):
    return Y.head_rows() if name == "big" else WT.head_input(name)


@gpu
@pytest.mark.parametrize("name,thresh", [(n, t) for n in ("small", "wide") for t in (0.0, 0.5, 0.9)] +
                         [("big", t) for t in Y.HEAD_THRESHOLDS])
def test_word_tree_top_is_the_walk_of_word_tree_head(name, thresh):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, tree = _walk_input(name)
    assert net.shape[0] % 4                                              # not a multiple of a workgroup's rows
    _out, ref_top, ref_prob, m = W.word_tree_head(net, tree, thresh, return_margins=True)
    assert m["thresh"] >= WT.MARGIN and m["group_gap"] >= WT.MARGIN, m
    tt = E.WordTreeTables(tree)
    src = dev(net)
    _rewritten, want_top, want_prob = E.word_tree_head(src, tt, thresh, want_top=True)
    top, prob = _top_with_guards(src, tt, thresh, None)
    assert np.array_equal(bits(src), net.view(np.uint32))                # net is not written
    assert np.array_equal(top, want_top.cpu().numpy()) and np.array_equal(bits(prob), bits(want_prob))
    assert np.array_equal(top, ref_top)
    np.testing.assert_allclose(prob, ref_prob, rtol=2e-5)
    # without prob: top alone, the same
    only = torch.full((net.shape[0],), -77, dtype=torch.int32, device="cuda")
    lib = E._lib.load()
    assert lib.y2_word_tree_top(ptr(src), ptr(tt.tables), net.shape[0], tree.n, tt.groups, tt.max_depth, thresh, -1.0,
                                ptr(only), None, None) == 0, lib.y2_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(only.cpu().numpy(), top)


@gpu
@pytest.mark.parametrize("name", ["wide", "big"])
def test_word_tree_top_skips_rows_below_the_objectness_threshold(name):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, tree = _walk_input(name)
    net = net.copy()
    obj, thresh = 0.3, 0.5 if name == "wide" else Y.DEPTH_THRESH
    # planted on both sides of so = 0.3 (to = log(0.3 / 0.7) = -0.8473), far on both sides, and a NaN
    planted = (-0.86, -0.83, -30.0, 30.0, np.nan, -0.8473 - 1e-3, -0.8473 + 1e-3)
    net[:len(planted), 4] = planted
    with np.errstate(all="ignore"):
        so = 1.0 / (1.0 + np.exp(-net[:, 4].astype(np.float64)))
        assert np.nanmin(np.abs(so - obj)) > 1e-5                        # float32 decides every row as float64 does
        walked = so > obj                                                # (NaN compares false)
    assert walked[:len(planted)].tolist() == [False, True, False, True, False, False, True]
    assert 20 < walked.sum() < len(walked) - 20
    tt = E.WordTreeTables(tree)
    src = dev(net)
    full_top, full_prob = _top_with_guards(src, tt, thresh, None)
    top, prob = _top_with_guards(src, tt, thresh, obj)
    assert (top[~walked] == -1).all() and (bits(prob[~walked]) == 0).all()        # -1 and +0.0f exactly
    assert np.array_equal(top[walked], full_top[walked]) and np.array_equal(bits(prob[walked]), bits(full_prob[walked]))
    assert (full_top >= 0).all()
    # the class logits of a skipped row are not read: filled with NaN they change nothing
    poisoned = net.copy()
    poisoned[~walked, 5:] = np.nan
    top2, prob2 = _top_with_guards(dev(poisoned), tt, thresh, obj)
    assert np.array_equal(top2, top) and np.array_equal(bits(prob2), bits(prob))
    assert np.array_equal(bits(src), net.view(np.uint32))


# ---- 3, 4: the rows
# (S, B, tree, images of tree_case): 125 candidates (KP 128), 845 (one slot per lane), 1805 (two), rows of 9,423 floats.
# The last one is a batch of 2 on purpose (38 MB): it leaves out image 1, the sized image with nothing above the
# threshold, which the three narrower geometries cover; at that width "no valid candidate" is the unsized table row
GEOMETRIES = ((5, 5, "small", (0, 1, 2)), (13, 5, "wide70", (0, 1, 2)), (19, 5, "wide70", (0, 1, 2)),
              (13, 3, "big", (0, 2)))
SCORE_THRESHOLDS, IOU_THRESHOLDS, MAX_OUT = (0.0, 0.005, 0.2), (0.0, 0.45, 1.0), 24
UNSIZED = len(SHAPES)                                                    # the table row added behind _table()'s


def _tables():
    import torch
    return torch.from_numpy(np.concatenate([_table(), np.zeros((1, 5), np.int64)])).cuda()


def _filled(n, m):
    import torch
    return (torch.full((n, m, 6), 77, dtype=torch.int32, device="cuda"),
            torch.full((n, m), 7.0, dtype=torch.float32, device="cuda"),
            torch.full((n,), 77, dtype=torch.int32, device="cuda"))


def _host(out):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same(a, b, what):
    assert np.array_equal(a[2], b[2]), (what, a[2], b[2])                 # count
    assert np.array_equal(a[0], b[0]), what                               # det, the -1 of unused rows included
    assert np.array_equal(bits(a[1]), bits(b[1])), what                   # score bits, the 0 of unused rows included


class _Case:
    """one geometry on the device: the raw head, its rewrite and top from the old entry, the decode the specification
    reads (the device's own boxes and sig(to))"""

    def __init__(self, S, B, name, images):
        import torch
        from tensorflow_yolo2_amd import engine as E
        self.E, self.S, self.B, self.tree = E, S, B, T.TREES[name]()
        net, self.named, self.nodes = T.tree_case(S, B, self.tree)
        self.n, self.K, self.C = len(images), S * S * B, self.tree.n
        self.images = images
        self.raw = dev(net[list(images)])
        self.tt = E.WordTreeTables(self.tree)
        self.rewritten, top, _prob = E.word_tree_head(self.raw, self.tt, T.TREE_THRESH, want_top=True)
        self.top, _prob = E.word_tree_top(self.raw, self.tt, T.TREE_THRESH)
        assert torch.equal(self.top, top)
        boxes, scores = E.decode_anchors(self.rewritten, ANCHORS[:B])
        so = scores.view(-1, self.C).gather(1, self.top.long()[:, None])
        del scores
        self.boxes = boxes.cpu().numpy().reshape(self.n, self.K, 4)
        self.so = so.cpu().numpy().reshape(self.n, self.K)
        self.top_h = self.top.cpu().numpy().reshape(self.n, self.K)
        self.table = _tables()

    def new(self, top, index, st, it, mo, net_size, protocol="repo", raw=None):
        idx = dev(np.asarray(index, np.int32)) if index is not None else None
        return _host(self.E.detect_anchor_tree_batch(self.raw if raw is None else raw, top, ANCHORS[:self.B], self.table,
                                                     idx, st, it, mo, out=_filled(self.n, mo), net_size=net_size,
                                                     protocol=protocol))

    def old(self, index, st, it, mo, net_size):
        idx = dev(np.asarray(index, np.int32)) if index is not None else None
        return _host(self.E.detect_anchor_batch(self.rewritten, ANCHORS[:self.B], self.table, idx, st, it, mo,
                                                out=_filled(self.n, mo), net_size=net_size))

    def spec(self, entries, st, it, mo, net_size, so=None, darknet=False):
        """the host specification on the device's decode, in the layout of the entries' outputs"""
        so = self.so if so is None else so
        det, score, count = (np.full((self.n, mo, 6), -1, np.int32), np.zeros((self.n, mo), np.float32),
                             np.zeros(self.n, np.int32))
        for k, e in enumerate(entries):
            if e == UNSIZED:
                continue                                                  # a table row without a size: no candidate is valid
            h, w = SHAPES[e]
            if darknet:
                d, s = DB.anchor_detect_tree_darknet(self.boxes[k], so[k], self.top_h[k], w, h, st, it, mo, net_size)
            else:
                d, s = DB.anchor_detect(self.boxes[k], so[k], self.top_h[k], w, h, st, it, mo, net_size=net_size)
            count[k] = len(d)
            det[k, :len(d)], score[k, :len(d)] = d, s
        return det, score, count


_CASES = {}


def _case(S, B, name, images):
    if (S, B, name) not in _CASES:
        _CASES.clear()                                                    # one geometry's tensors on the device at a time
        _CASES[S, B, name] = _Case(S, B, name, images)
    return _CASES[S, B, name]


def _entries(c, with_index):
    """(entries of the slots, the index argument): the first n table rows, or other sizes and the unsized row"""
    if not with_index:
        return tuple(range(c.n)), None
    index = (2, UNSIZED, 0)[:c.n]
    return index, index


@gpu
@pytest.mark.parametrize("S,B,name,images", GEOMETRIES)
def test_integer_tree_rows_equal_the_old_two_launches_and_the_specification(S, B, name, images):
    """E1 and E2 over every variant on the device; the specification at three (score, IoU, cap) triples that meet every
    value once, each under stretch and letterbox, with and without an index"""
    import torch
    c = _case(S, B, name, images)
    E, K, N = c.E, c.K, 32 * S
    assert K not in (64, 128, 256, 512, 1024, 2048)
    # the inputs make the specification suppress a_same (the node of a) and keep a_other (another node)
    named, top0 = c.named, c.top_h[0]
    for cand, node in c.nodes.items():
        assert top0[named[cand]] == node, cand
    assert len(set(top0.tolist())) > 3
    h, w = SHAPES[0]
    kept = DB.anchor_detect(c.boxes[0], c.so[0], top0, w, h, 0.2, 0.45, K)[0][:, 5].tolist()
    assert named["a"] in kept and named["a_same"] not in kept and named["a_other"] in kept
    assert np.isnan(c.so[0][named["nan_to"]])
    skipped = {st: E.word_tree_top(c.raw, c.tt, T.TREE_THRESH, st)[0] for st in SCORE_THRESHOLDS}
    assert (skipped[0.2] == -1).sum().item() > K // 4                     # E2's top does skip rows
    checked = 0
    for net_size, with_index, st, it, mo in itertools.product((None, N), (False, True), SCORE_THRESHOLDS, IOU_THRESHOLDS,
                                                              (MAX_OUT, K)):
        entries, index = _entries(c, with_index)
        what = (net_size, index, st, it, mo)
        old = c.old(index, st, it, mo, net_size)
        new = c.new(c.top, index, st, it, mo, net_size)
        _same(new, old, ("E1",) + what)
        _same(c.new(skipped[st], index, st, it, mo, net_size), old, ("E2",) + what)
        if (st, it, mo) in ((0.2, 0.45, MAX_OUT), (0.0, 0.0, K), (0.005, 1.0, K)):    # under every net_size / index pairing
            _same(new, c.spec(entries, st, it, mo, net_size), ("spec",) + what)
            checked += 1
        if with_index and c.n == 3:
            assert new[2][1] == 0                                         # the unsized row
    assert checked == 12
    first = c.new(c.top, None, 0.2, 0.45, MAX_OUT, None)[2]
    assert 0 < first[0] and first[-1] == MAX_OUT and (c.n < 3 or first[1] == 0)   # rows kept, nothing, an overflow
    assert c.new(c.top, None, 0.2, 0.45, K, None)[2][-1] > MAX_OUT
    # a negative threshold: against the specification only (the old entry gives a zero-score candidate class 0)
    for net_size in (None, N):
        _same(c.new(c.top, None, -1.0, 0.45, K, net_size), c.spec(range(c.n), -1.0, 0.45, K, net_size), ("negative", net_size))
    # a top outside [0, C) in three live candidates drops exactly those
    before = c.new(c.top, None, 0.2, 0.45, K, None)
    assert before[2][0] > 3
    live = before[0][0, :3, 5].tolist()                                   # the three best kept rows of image 0
    bad = c.top.clone()
    bad[torch.tensor(live, device="cuda")] = torch.tensor([-1, c.C, INT_MAX], dtype=torch.int32, device="cuda")
    so = c.so.copy()
    so[0, live] = np.nan                                                  # the specification's way to say "not valid"
    after = c.new(bad, None, 0.2, 0.45, K, None)
    _same(after, c.spec(range(c.n), 0.2, 0.45, K, None, so=so), "bad top")
    assert not set(live) & set(after[0][0, :after[2][0], 5].tolist())
    # nothing behind element 4 of a row is read: the class logits filled with NaN give the same bits
    poisoned = c.raw.clone()
    poisoned[..., 5:] = float("nan")
    _same(c.new(c.top, None, 0.2, 0.45, K, None, raw=poisoned), before, "poisoned")
    _same(c.new(c.top, None, 0.2, 0.45, MAX_OUT, N, protocol="darknet", raw=poisoned),
          c.new(c.top, None, 0.2, 0.45, MAX_OUT, N, protocol="darknet"), "poisoned dk")


@gpu
@pytest.mark.parametrize("S,B,name,images", [g for g in GEOMETRIES if g[:2] in ((13, 5), (19, 5))])
def test_darknet_tree_rows_equal_the_per_class_segments_and_the_specification(S, B, name, images):
    """E3, the specification with and without a binding max_out, and the float matcher on the flat rows"""
    import torch
    c = _case(S, B, name, images)
    E, K, N, C = c.E, c.K, 32 * S, c.C
    table = c.table
    for st, it in ((0.2, 0.45), (0.0, 0.0), (0.005, 1.0)):
        flat = c.new(c.top, None, st, it, K, N, protocol="darknet")
        _same(flat, c.spec(range(c.n), st, it, K, N, darknet=True), ("dk spec", st, it))
        seg = _host(E.detect_anchor_classes_batch_darknet(c.rewritten, ANCHORS[:B], table, None, st, it, K, net_size=N))
        for k in range(c.n):
            rows, scores = flat[0][k, :flat[2][k]], flat[1][k, :flat[2][k]]
            assert flat[2][k] == seg[2][k].sum(), (k, st, it)
            for node in np.nonzero(seg[2][k])[0]:
                sel, cnt = rows[:, 4] == node, seg[2][k, node]
                assert np.array_equal(rows[sel], seg[0][k, node, :cnt]), (k, node)
                assert np.array_equal(bits(scores[sel]), bits(seg[1][k, node, :cnt])), (k, node)
    index = (2, UNSIZED, 0)
    capped = c.new(c.top, index, 0.2, 0.45, MAX_OUT, N, protocol="darknet")
    _same(capped, c.spec(index, 0.2, 0.45, MAX_OUT, N, darknet=True), "dk capped")
    assert capped[2][2] == MAX_OUT and capped[2][1] == 0                  # the overflowing image; the unsized row
    # the rows as y2_voc_match_batch_f reads them: hand-made truths of the kept rows' own nodes
    det, score, count = (dev(a) for a in c.new(c.top, None, 0.2, 0.45, MAX_OUT, N, protocol="darknet"))
    det_h, count_h = det.cpu().numpy(), count.cpu().numpy()
    max_obj = 4
    boxes = np.zeros((len(SHAPES), max_obj, 5), np.float64)
    counts = np.zeros(len(SHAPES), np.int32)
    difficult = np.zeros((len(SHAPES), max_obj), np.uint8)
    for k in range(c.n):
        picks = det_h[k, :count_h[k]][:max_obj]
        for j, row in enumerate(picks):                                  # a truth on each of the first kept rows
            corners = np.ascontiguousarray(row[:4]).view(np.float32).astype(np.float64)
            boxes[k, j] = tuple(np.round(corners)) + (row[4],)
        counts[k] = len(picks)
        if len(picks):                                                    # the largest of them is difficult
            difficult[k, np.argmax((boxes[k, :len(picks), 2] - boxes[k, :len(picks), 0]) *
                                   (boxes[k, :len(picks), 3] - boxes[k, :len(picks), 1]))] = 1
    flags = E.voc_match_batch_f(det, score, count, dev(boxes), dev(counts), dev(difficult), None, 0.5)
    flags = flags.cpu().numpy()
    for k in range(c.n):
        want = DB.match_image_f(det_h[k, :count_h[k]], boxes[k, :counts[k]], difficult[k, :counts[k]], 0.5)
        assert np.array_equal(flags[k, :count_h[k]], want) and (flags[k, count_h[k]:] == -1).all(), k
    assert (flags == 1).any() and (flags == 2).any() and (flags == 0).any()


# ---- 5: argument errors
@gpu
def test_tree_entries_reject_bad_arguments_and_launch_nothing():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = ptr(buf)
    before = buf.clone()
    inf, nan = float("inf"), float("nan")
    #        net tables rows C  G  depth tree_thresh obj_thresh top prob
    good = [p, p, 12, 20, 7, 2, 0.5, -1.0, p, p, None]
    for at, value, word in ((8, None, b"null"), (0, None, b"null"), (1, None, b"null"), (7, inf, b"obj_thresh"),
                            (7, -inf, b"obj_thresh"), (7, nan, b"obj_thresh"), (6, 1.0, b"tree_thresh"),
                            (6, -0.1, b"tree_thresh"), (2, 0, b"rows"), (2, -4, b"rows"), (3, 0, b"num_class"),
                            (4, 21, b"G = 21"), (5, 20, b"max_depth")):
        a = list(good)
        a[at] = value
        assert lib.y2_word_tree_top(*a) == -1, (at, value)
        err = lib.y2_last_error()
        assert b"y2_word_tree_top" in err and word in err, (at, value, err)
    for name in ("y2_detect_anchor_tree_batch", "y2_detect_anchor_tree_batch_dk"):
        entry = getattr(lib, name)
        #     net top anchors table index n  S   B  C  score iou max_out net_size det score count
        good = [p, p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, 416, p, p, p, None]
        cases = [(1, None, b"null"), (0, None, b"null"), (2, None, b"null"), (3, None, b"null"), (13, None, b"null"),
                 (14, None, b"null"), (15, None, b"null"), (12, 100, b"net_size = 100"), (12, 448, b"net_size = 448"),
                 (12, -416, b"net_size = -416"), (6, 21, b"S * S * B = 2205"), (7, 17, b"B = 17"), (8, 0, b"num_class = 0"),
                 (5, 0, b"n = 0"), (11, 0, b"max_out = 0")]
        if name.endswith("_dk"):
            cases.append((12, 0, b"net_size = 0"))                        # Darknet's protocol is letterboxed
        for at, value, word in cases:
            a = list(good)
            a[at] = value
            if at == 6:
                a[12] = 32 * value
            assert entry(*a) == -1, (name, at, value)
            err = lib.y2_last_error()
            assert name.encode() + b":" in err and word in err, (name, at, value, err)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


# ---- 6: the detector
def _wide_detector(tmp_path, which, n=2):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    if which == "wide700":
        cfg = WH.write_wide_model_files(tmp_path)
        det = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16", seed=3, wide_head=True)
    else:
        cfg = Y.write_yolo9000_width_files(tmp_path)
        det = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16", seed=3, wide_head=True,
                                             tree_thresh=Y.DETECTOR_TREE_THRESH)
    weights = WH.random_weights_file(str(tmp_path / "wide.weights"), det.cfg.file_layers, seed=Y.DETECTOR_WEIGHTS_SEED)
    assert net_utils.load_darknet_weights(det, weights) == 1234
    return det, cfg, weights


def _darknet_rows_on_the_host(E, det, grids, shapes, thresh, iou, max_out):
    """anchor_detect_tree_darknet per image on the device's decode of `grids` [m,S,S,B,5+C] (raw heads) ->
    [(det rows, scores)]"""
    rewritten, top, _prob = E.word_tree_head(grids.contiguous(), det.tree, det.tree_thresh, want_top=True)
    boxes, scores = E.decode_anchors(rewritten, det.anchors)
    m = grids.shape[0]
    so = scores.view(-1, det.num_class).gather(1, top.long()[:, None]).cpu().numpy().reshape(m, -1)
    boxes, top = boxes.cpu().numpy().reshape(m, -1, 4), top.cpu().numpy().reshape(m, -1)
    return [DB.anchor_detect_tree_darknet(boxes[k], so[k], top[k], shapes[k][1], shapes[k][0], thresh, iou, max_out,
                                          det.size) for k in range(m)]


@gpu
@pytest.mark.parametrize("which,C", (("wide700", 700), ("yolo9000", 9418)))
def test_wide_detector_detects_from_the_node(tmp_path, which, C):
    import torch
    from tensorflow_yolo2_amd import engine as E
    n, S, thresh, iou, max_out = 2, 5, 0.05, 0.45, 20
    det, _cfg, _weights = _wide_detector(tmp_path, which)
    assert det.wide is not None and det.num_class == C == det.tree.n
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8))
    table = torch.from_numpy(_table()).cuda()
    for letterbox in (False, True):
        raw = torch.full((n, S, S, 3, 5 + C), float("nan"), device="cuda")
        got = _host(det.detect_batch(x, table, None, thresh, iou, max_out, grid_out=raw, letterbox=letterbox))
        again = det.forward(x)
        assert torch.equal(raw.view(torch.int32), again.view(torch.int32)) and torch.isfinite(raw).all()   # still the raw head
        old = _host(E.detect_anchor_batch(E.word_tree_head(raw, det.tree, det.tree_thresh), det.anchors_dev, table, None,
                                          thresh, iou, max_out, net_size=160 if letterbox else None))
        _same(got, old, letterbox)
        assert got[2].sum() > 0
        _same(_host(det.detect_tree_batch(x, table, None, thresh, iou, max_out, letterbox=letterbox)), old, letterbox)
    # Darknet's rows from a float batch
    xf = dev(np.random.default_rng(9).random((n, 160, 160, 3), dtype=np.float32))
    raw = torch.empty((n, S, S, 3, 5 + C), device="cuda")
    d, s, c = _host(det.detect_tree_batch(xf, table, None, thresh, iou, max_out, grid_out=raw, letterbox=True,
                                          protocol="darknet"))
    want = _darknet_rows_on_the_host(E, det, raw, SHAPES, thresh, iou, max_out)
    for k, (wd, ws) in enumerate(want):
        assert c[k] == len(wd) and np.array_equal(d[k, :c[k]], wd) and np.array_equal(bits(s[k, :c[k]]), bits(ws)), k
        assert (d[k, c[k]:] == -1).all() and (s[k, c[k]:] == 0).all()
    assert c.sum() > 0 and len(set(np.concatenate([d[k, :c[k], 4] for k in range(n)]).tolist())) > 1
    # what stays refused, and what detect_tree_batch refuses
    with pytest.raises(ValueError, match="detect_batch"):
        det.detect_classes_batch(x, table, None, thresh, iou, 8)
    with pytest.raises(ValueError, match="letterbox=True"):
        det.detect_tree_batch(xf, table, None, thresh, iou, max_out, protocol="darknet")
    with pytest.raises(ValueError, match="neither"):
        det.detect_tree_batch(x, table, None, thresh, iou, max_out, protocol="other")


@gpu
def test_narrow_models_keep_their_paths(monkeypatch):
    """chain-tree.cfg: detect_classes_batch is what it was, through the rewrite and not through word_tree_top; a model
    without a tree refuses detect_tree_batch and its detect_batch launches what it launched"""
    import torch
    from test_gpu_detect_anchor import _unit_gain_layers
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, thresh, iou, per_class = 2, 0.005, 0.45, 8
    det = yolov2.YOLOv2Detector.from_cfg(WT.CHAIN_TREE_CFG, n, dtype="f32", seed=4)
    for net in det.networks():
        net.load_params(_unit_gain_layers(net))
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 64, 64, 3), dtype=np.uint8))
    table = torch.from_numpy(_table()).cuda()
    tree_rows = _host(det.detect_tree_batch(x, table, None, thresh, iou, 12))
    _same(_host(det.detect_batch(x, table, None, thresh, iou, 12)), tree_rows, "narrow detect_batch")
    raw = det.forward(x).clone()
    want = _host(E.detect_anchor_classes_batch(E.word_tree_head(raw, det.tree, det.tree_thresh), det.anchors_dev, table,
                                               None, thresh, iou, per_class))

    def refuse(*a, **kw):
        raise AssertionError("word_tree_top on the per-class path")
    monkeypatch.setattr(E, "word_tree_top", refuse)
    got = _host(det.detect_classes_batch(x, table, None, thresh, iou, per_class))
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
    assert want[2].sum() > 0
    # below a negative threshold detect_batch keeps the rewrite (a zero-score candidate's class is 0 there)
    det.detect_batch(x, table, None, -1.0, iou, 12)
    flat = yolov2.YOLOv2Detector(n, 224, dtype="f32", width_div=8, seed=4)
    x224 = dev(np.random.default_rng(8).integers(0, 256, (n, 224, 224, 3), dtype=np.uint8))
    flat.detect_batch(x224, table, None, thresh, iou, 12)                 # no tree: no walk at all
    with pytest.raises(ValueError, match="word tree"):
        flat.detect_tree_batch(x224, table, None, thresh, iou, 12)


# ---- 7: end to end
@gpu
def test_evaluate_yolov2_scores_a_wide_model_under_darknets_protocol(tmp_path, golden_dir):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.pascal.pascal_eval_yolov2 import evaluate_yolov2
    det, _cfg, _weights = _wide_detector(tmp_path, "wide700")
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir)           # the two golden images: one batch
    imdb = DeviceVOC("trainval", batch_size=2, devkit_path=kit, flipped=False)
    thresh, iou, max_out = 0.02, 0.45, 30
    r = evaluate_yolov2(det, imdb, 160, thresh, iou, max_out, True, True, True, 32, True, 127, protocol="darknet")
    assert r["tree_rows"] and r["count"].shape == (2,) and r["saturated"] == int((r["count"] >= max_out).sum())
    assert tuple(r["grids"].shape) == (2, 5, 5, 3, 705) and torch.isfinite(r["grids"]).all()   # the raw heads
    want = _darknet_rows_on_the_host(E, det, r["grids"], [e["shape"] for e in imdb.entries], thresh, iou, max_out)
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    for k, (wd, ws) in enumerate(want):
        e = imdb.entries[k]
        rows["image"] += [k] * len(wd)
        rows["box"] += np.ascontiguousarray(wd[:, :4]).view(np.float32).tolist()
        rows["class"] += wd[:, 4].tolist()
        rows["candidate"] += wd[:, 5].tolist()
        rows["score"] += ws.tolist()
        rows["flag"] += DB.match_image_f(wd, np.asarray(e["objs"], np.float64), e["difficult"], 0.5).tolist()
    assert len(rows["image"]) > 4 and set(rows["image"]) == {0, 1}
    for key in rows:
        assert r["rows"][key].tolist() == rows[key], key
    assert r["count"].tolist() == [rows["image"].count(k) for k in range(2)]
    assert np.isfinite(r["mAP"]) and sorted(r["aps"]) == sorted(r["npos"])
    # the keyword: a narrow tree model keeps per-class segments unless it is set; a wide one cannot take them
    with pytest.raises(ValueError, match="detect_batch"):
        evaluate_yolov2(det, imdb, 160, thresh, iou, max_out, True, False, True, 32, True, 127, protocol="darknet",
                        tree_rows=False)
    plain = evaluate_yolov2(det, imdb, 160, thresh, iou, max_out, True, False, True, 32, False, 127)   # per_class, repo
    assert plain["tree_rows"] and plain["count"].shape == (2,) and plain["rows"]["box"].dtype == np.int32


@gpu
def test_detector_map_and_valid_and_the_detect_script_on_a_wide_cfg(tmp_path, golden_dir, capsys):
    import torch
    from test_gpu_device_darknet import make_list
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.darknet import detector
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2
    root = str(tmp_path)
    det, cfg, weights = _wide_detector(tmp_path, "wide700")
    del det
    lst = make_list(root, golden_dir)
    data = os.path.join(root, "wide.data")
    with open(data, "w") as f:
        f.write("classes = 700\nvalid = %s\nresults = %s\n" % (lst, os.path.join(root, "results")))
    flags = ["--batch", "2", "--size", "160", "--dtype", "f16", "--thresh", "0.02"]
    res = detector.main(["map", data, cfg, weights] + flags)
    out = capsys.readouterr().out
    assert np.isfinite(res["mAP"]) and res["tree_rows"] and len(res["imdb"].entries) == 6 and "Mean AP = " in out
    assert "images reached --max-out 100" in out and res["count"].shape == (6,)
    assert len(res["rows"]["score"]) > 0 and sorted(res["aps"]) == sorted(res["npos"])
    res = detector.main(["valid", data, cfg, weights] + flags)
    files = res["results_files"]
    assert len(files) == 700 and all(os.path.dirname(p) == os.path.join(root, "results") for p in files)
    lines = [ln.split() for p in files for ln in open(p).read().splitlines()]
    assert len(lines) == len(res["rows"]["score"]) > 0 and all(len(ln) == 6 and ln[0].startswith("im") for ln in lines)
    # the detect script: Darknet's lines from the flat rows of the same entry on the kept heads
    capsys.readouterr()
    images = [os.path.join(root, "images", "im%d.png" % k) for k in range(3)]
    r = pascal_detect_yolov2.main(["--cfg", cfg, "--darknet-weights", weights, "--images"] + images +
                                  ["--batch", "2", "--size", "160", "--dtype", "f16", "--thresh", "0.02", "--max-out", "30",
                                   "--protocol", "darknet", "--keep-grids"])
    printed = capsys.readouterr().out.splitlines()
    pool, model = r["pool"], r["detector"]
    assert tuple(r["grids"].shape) == (3, 5, 5, 3, 705)
    shapes = [(int(h), int(w)) for (_o, h, w, _p, _f) in pool.table.cpu().numpy().tolist()]
    want = _darknet_rows_on_the_host(E, model, r["grids"], shapes, 0.02, 0.45, 30)
    lines = []
    for k, (wd, ws) in enumerate(want):
        for row, s in zip(wd, ws):
            corners = np.ascontiguousarray(row[:4]).view(np.float32)
            lines.append("%s %s %f %f %f %f %f" % ((images[k], model.tree.tree.labels[row[4]], float(s)) +
                                                   tuple(float(v) for v in corners)))
    assert len(lines) > 3 and [ln for ln in printed if ln.startswith(root)] == lines
