"""The word tree on the GPU (csrc/word_tree.hip) against the float64 specification (utils/word_tree.py):
y2_yolov2_loss_boxes_tree, y2_yolov2_region_stats_tree and y2_word_tree_head, a detector and a trainer built from
tests/golden/cfg/chain-tree.cfg, and the argument errors of the three entries.

Float32 and float64 may decide differently at a tie, so every parity input asserts on the CPU, before the device call,
that the specification's decision margins are at least 1e-5 (tests/test_gpu_region_loss.py's method; the seeds of
tests/_word_tree_cases.py were fixed so that this holds).  Tolerances are that file's: loss rtol 2e-5, largest gradient
error / largest gradient < 2e-5; the statistics' rtol 2e-5 (tests/test_gpu_region_stats.py); prob rtol 2e-5."""
import ctypes

import numpy as np
import pytest

import _word_tree_cases as K
from tensorflow_yolo2_amd.utils import detect_batch as DB, word_tree as W

gpu = pytest.mark.gpu
RTOL = 2e-5


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def assert_close(loss, dnet, ref_loss, ref_d):
    print("loss", loss, "reference", ref_loss)
    np.testing.assert_allclose(loss, ref_loss, rtol=RTOL)
    if dnet is not None:
        err = np.abs(dnet - ref_d).max() / np.abs(ref_d).max()
        print("largest gradient error / largest gradient", err)
        assert err < 2e-5, err


@gpu
@pytest.mark.parametrize("key", sorted(K.SHAPES))
def test_tree_loss_matches_the_float64_specification(key):
    K.check_tree_loss_on_the_device(K.parity_input(key))


@gpu
@pytest.mark.parametrize("key", ["n3_S5_small", "n2_S8_B3_wide"])
def test_tree_stats_match_the_float64_specification(key):
    K.check_tree_stats_on_the_device(K.parity_input(key))


@gpu
@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("thresh", [0.0, 0.5, 0.9])
def test_word_tree_head_matches_the_specification(name, thresh):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, tree = K.head_input(name)
    assert net.shape[0] % 4                                              # not a multiple of a workgroup's rows
    ref_out, ref_top, ref_prob, m = W.word_tree_head(net, tree, thresh, return_margins=True)
    assert m["thresh"] >= K.MARGIN and m["group_gap"] >= K.MARGIN, m
    tt = E.WordTreeTables(tree)
    src = dev(net)
    out = torch.full(net.shape, 7.0, device="cuda")
    got, top, prob = E.word_tree_head(src, tt, thresh, out=out, want_top=True)
    assert got is out and np.array_equal(bits(src), net.view(np.uint32))  # the input is not written
    o = out.cpu().numpy()
    assert np.array_equal(top.cpu().numpy(), ref_top)
    assert np.array_equal(o[:, :5].view(np.uint32), net[:, :5].view(np.uint32))
    assert ((o[:, 5:] == 0).sum(axis=1) == 1).all() and (np.isneginf(o[:, 5:]).sum(axis=1) == tree.n - 1).all()
    assert np.array_equal(o.view(np.uint32), ref_out.view(np.uint32))    # the 0 is +0.0 and stands at top
    err = np.abs(prob.cpu().numpy() - ref_prob) / ref_prob
    print("word_tree_head %s thresh %.1f: largest relative error of prob %.3e" % (name, thresh, err.max()))
    np.testing.assert_allclose(prob.cpu().numpy(), ref_prob, rtol=RTOL)
    # in place, and without the optional outputs: the same bits
    same = E.word_tree_head(src, tt, thresh, out=src)
    assert same is src and np.array_equal(bits(src), bits(out))


@gpu
def test_detector_rows_with_a_tree_are_the_specification_on_the_rewritten_head():
    """a width_div model from chain-tree.cfg at its 64 x 64 input: detect_classes_batch with the tree, bit for bit against
    utils/detect_batch.anchor_detect_classes on the device-decoded boxes and the scores sig(to) * onehot(top)"""
    import torch
    from test_gpu_detect_anchor import SHAPES, _table, _unit_gain_layers
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, thresh, iou, per_class = 2, 0.005, 0.45, 8
    det = yolov2.YOLOv2Detector.from_cfg(K.CHAIN_TREE_CFG, n, dtype="f32", seed=4)
    assert det.tree is not None and det.tree.n == 20 == det.num_class and det.tree_thresh == 0.4 and det.B == 3
    for net in det.networks():
        net.load_params(_unit_gain_layers(net))
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 64, 64, 3), dtype=np.uint8))
    table = torch.from_numpy(_table()).cuda()
    raw = torch.empty((n, 2, 2, 3, 25), dtype=torch.float32, device="cuda")
    rows, score, count = det.detect_classes_batch(x, table, None, thresh, iou, per_class, grid_out=raw)
    torch.cuda.synchronize()
    head = raw.cpu().numpy().reshape(-1, 25)
    _out, top, _prob, m = W.word_tree_head(head, det.tree.tree, det.tree_thresh, return_margins=True)
    assert min(m.values()) >= K.MARGIN, m
    assert len(set(top.tolist())) > 1
    boxes, so_all = E.decode_anchors(E.word_tree_head(raw, det.tree, det.tree_thresh), det.anchors)
    boxes, so_all = boxes.cpu().numpy(), so_all.cpu().numpy()
    so = so_all.reshape(-1, 20)[np.arange(len(top)), top]                # the device's sig(to)
    scores = np.zeros((len(top), 20), np.float32)
    scores[np.arange(len(top)), top] = so
    assert np.array_equal(scores.view(np.uint32), so_all.reshape(-1, 20).view(np.uint32))   # so * 1 at top, so * 0 elsewhere
    np.testing.assert_allclose(so, 1.0 / (1.0 + np.exp(-head[:, 4].astype(np.float64))), rtol=1e-6)
    scores = scores.reshape(n, -1, 20)
    for k in range(n):
        want = DB.anchor_detect_classes(boxes[k], scores[k], SHAPES[k][1], SHAPES[k][0], thresh, iou, per_class)
        assert np.array_equal(count[k].cpu().numpy(), want[2])
        assert np.array_equal(rows[k].cpu().numpy(), want[0])
        assert np.array_equal(bits(score[k]), want[1].view(np.uint32))
    assert count.sum().item() > 0
    # detect() decodes the same head: every candidate's class is its node, its best score the objectness
    _boxes, best, cls, _keep, _count = det.detect(x)
    assert np.array_equal(cls.cpu().numpy().ravel(), top) and np.array_equal(bits(best).ravel(), so.view(np.uint32))
    # detect_batch reads the same head: its classes are the tree's nodes
    d, _s, c = det.detect_batch(x, table, None, thresh, iou, 12)
    kept = d.cpu().numpy()[0, :int(c[0])]
    assert len(kept) and set(kept[:, 4].tolist()) <= set(top[:12].tolist())


@gpu
def test_trainer_step_with_a_tree():
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    batch, size = 2, 64
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(K.CHAIN_TREE_CFG, dtype="f32", seed=5)
    assert tr.tree is not None and tr.batch == batch and tr.tree_thresh == 0.4
    x = dev(np.random.default_rng(3).integers(0, 256, (batch, size, size, 3), dtype=np.uint8))
    truth = np.zeros((batch, 30, 5), np.float32)
    for i in range(batch):
        truth[i, 0] = (21.0, 26.0, 23.0, 29.0, 18 + i)                   # leaves of depth 2
        truth[i, 1] = (44.0, 39.0, 20.0, 18.0, 4 * i)                    # inner nodes: animal, dog
    td, cd = dev(truth), dev(np.full(batch, 2, np.int32))
    with pytest.raises(ValueError, match="word tree"):
        tr.step(x, labels=torch.zeros((batch, 2, 2, 25), device="cuda"))
    assert tr.iteration == 0
    grid, _fine = tr.forward(x, True)                                    # the pass the step is about to run
    grid = grid.contiguous().clone()
    want_loss, want_d = E.yolov2_loss_boxes_tree(grid, td, cd, tr.anchors, size, tr.tree, True, tr.box_scales(1))
    want_stats = E.yolov2_region_stats_tree(grid, td, cd, tr.anchors, size, tr.tree)
    stats = torch.full((6,), float("nan"), device="cuda")
    loss = tr.step(x, truth=td, ntruth=cd, stats=stats)
    torch.cuda.synchronize()
    assert np.array_equal(bits(loss), bits(want_loss)) and np.array_equal(bits(tr.last_dnet), bits(want_d))
    assert np.array_equal(bits(stats), bits(want_stats))
    ref_loss, ref_d = W.yolov2_loss_boxes_tree(grid.cpu().numpy(), truth, [2, 2], tr.anchors, size, tr.tree.tree,
                                               area_weight=True, prior_scale=tr.prior_scale, **dict(tr.scales))
    assert_close(loss.cpu().numpy(), tr.last_dnet.cpu().numpy(), ref_loss, ref_d)
    flat_loss, _ = E.yolov2_loss_boxes(grid, td, cd, tr.anchors, size, False, tr.box_scales(1))
    assert float(flat_loss[3]) != float(loss[3]) and np.array_equal(bits(flat_loss)[:3], bits(loss)[:3])
    for net in tr.nets:
        assert torch.isfinite(net.params).all()


@gpu
def test_word_tree_entries_reject_bad_arguments():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    net, truth, ntruth, anchors, size, tree = K.parity_input("n3_S5_small")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    nd, td, cd, ad = dev(net), dev(truth), dev(ntruth), dev(np.asarray(anchors, np.float32))
    tb = dev(W.pack(tree))
    loss = torch.full((5,), float("nan"), device="cuda")
    stats = torch.full((6,), float("nan"), device="cuda")
    out = torch.full(net.shape, 7.0, device="cuda")
    ws = torch.empty(lib.y2_yolov2_loss_boxes_tree_workspace_bytes(3, 5, 5), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty(lib.y2_yolov2_region_stats_workspace_bytes(3), dtype=torch.uint8, device="cuda")
    common = (("net", p(nd)), ("truth", p(td)), ("ntruth", p(cd)), ("anchors", p(ad)), ("tables", p(tb)), ("batch", 3),
              ("S", 5), ("B", 5), ("C", 20), ("G", 7), ("depth", 2), ("T", 30), ("size", 160.0))
    entries = {
        "y2_yolov2_loss_boxes_tree": common + (("scales", None), ("loss", p(loss)), ("dnet", None), ("ws", p(ws)),
                                               ("stream", None)),
        "y2_yolov2_region_stats_tree": common + (("stats", p(stats)), ("ws", p(ws2)), ("stream", None)),
        "y2_word_tree_head": (("net", p(nd)), ("tables", p(tb)), ("rows", 3 * 5 * 5 * 5), ("C", 20), ("G", 7), ("depth", 2),
                              ("thresh", 0.5), ("out", p(out)), ("top", None), ("prob", None), ("stream", None)),
    }
    tree_cases = ((dict(tables=None), b"null"), (dict(net=None), b"null"), (dict(C=0), b"num_class"),
                  (dict(C=65537), b"num_class"), (dict(G=0), b"G = 0"), (dict(G=21), b"G = 21"),
                  (dict(depth=-1), b"max_depth"), (dict(depth=20), b"max_depth"))
    more = {"y2_yolov2_loss_boxes_tree": ((dict(truth=None), b"null"), (dict(ntruth=None), b"null"), (dict(anchors=None), b"null"),
                                          (dict(loss=None), b"null"), (dict(ws=None), b"null"), (dict(T=1025), b"max_boxes"),
                                          (dict(S=1024, B=2), b"MAX_SLOTS"), (dict(batch=0), b"batch")),
            "y2_yolov2_region_stats_tree": ((dict(truth=None), b"null"), (dict(stats=None), b"null"), (dict(ws=None), b"null"),
                                            (dict(T=0), b"max_boxes"), (dict(B=9), b"B = 9"), (dict(size=0.0), b"image_size")),
            "y2_word_tree_head": ((dict(out=None), b"null"), (dict(rows=0), b"rows"), (dict(thresh=1.0), b"tree_thresh"),
                                  (dict(thresh=-0.1), b"tree_thresh"))}
    for name, table in entries.items():
        call = lambda **kw: getattr(lib, name)(*[kw.get(k, v) for k, v in table])
        for kw, word in tree_cases + more[name]:
            assert call(**kw) == -1, (name, kw)                           # Y2_ERR_ARG
            err = lib.y2_last_error()
            assert name.encode() in err and word in err, (name, kw, err)
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(stats).all() and (out == 7.0).all()   # nothing was launched
    assert lib.y2_yolov2_loss_boxes_tree_workspace_bytes(3, 1024, 2) == 0
    for name, table in entries.items():
        assert getattr(lib, name)(*[v for _k, v in table]) == 0, name
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and torch.isfinite(stats).all() and not (out == 7.0).any()
