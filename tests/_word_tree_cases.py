"""Inputs shared by tests/test_word_tree_host.py and tests/test_gpu_word_tree.py: the trees, the parity inputs of the loss
and the statistics, the head rows.  Everything is generated on the CPU from fixed seeds; the seeds were chosen so that the
float64 specification's decision margins are at least 1e-5 (the tests assert it before any device call)."""
import os

import numpy as np

from tensorflow_yolo2_amd.utils import word_tree as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_TREE = os.path.join(ROOT, "tests", "golden", "tree", "small.tree")
CHAIN_TREE_CFG = os.path.join(ROOT, "tests", "golden", "cfg", "chain-tree.cfg")
VOC = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))
THREE = ((1.0, 1.5), (2.5, 3.0), (5.0, 4.0))
NONDEFAULT = dict(coord_scale=2.0, object_scale=3.0, noobject_scale=0.5, class_scale=1.5, thresh=0.4)
MARGIN = 1e-5


def wide_tree():
    """70 nodes, three levels: 3 roots; the 65 children of root 0 (a group wider than a wave); one child of root 1 and one
    child of node 3 (two groups of one).  5 + 70 = 75 floats per row: odd, so rows are not 16-byte aligned"""
    lines = ["r%d -1" % i for i in range(3)] + ["w%d 0" % i for i in range(65)] + ["single 1", "deep 3"]
    return W.parse("\n".join(lines) + "\n", "<wide>")


def small_tree():
    return W.load(SMALL_TREE)


# key -> (n, S, anchors, tree, seed, index of an image left without truths or None)
SHAPES = {"n3_S5_small": (3, 5, VOC, small_tree, 11, 1),
          "n2_S8_B3_wide": (2, 8, THREE, wide_tree, 3, None),
          "n1_S19_small": (1, 19, VOC, small_tree, 13, None)}


def parity_input(key):
    """(net, truth [n][30][5], ntruth, anchors, size, tree): image 0 carries 30 truths, most of them in four cells; the
    others a few.  A truth's class is any node of the tree, inner ones included"""
    n, S, anchors, make_tree, seed, empty = SHAPES[key]
    tree = make_tree()
    B, C = len(anchors), tree.n
    rng = np.random.default_rng(seed)
    size = 32 * S
    net = (rng.standard_normal((n, S, S, B, 5 + C)) * 0.7).astype(np.float32)
    truth = np.zeros((n, 30, 5), np.float32)
    ntruth = np.zeros(n, np.int32)
    an = np.asarray(anchors)
    for i in range(n):
        k = 30 if i == 0 else (0 if i == empty else int(rng.integers(2, 6)))
        which = rng.integers(0, B, k)
        scale = rng.uniform(0.75, 1.3, (k, 2))
        hot = rng.integers(0, S, (4, 2))                       # image 0: most centres fall into four cells
        cell = hot[rng.integers(0, 4, k)] if i == 0 else rng.integers(0, S, (k, 2))
        centre = (cell + rng.uniform(0.05, 0.95, (k, 2))) * 32.0
        truth[i, :k, 0:2] = centre
        truth[i, :k, 2:4] = np.minimum(an[which] * scale * 32.0 * S / 13.0 if B == 5 else an[which] * scale * 32.0, size - 1.0)
        truth[i, :k, 4] = rng.integers(0, C, k)
        ntruth[i] = k
    return net, truth, ntruth, anchors, size, tree


def checked_loss(net, truth, ntruth, anchors, size, tree, **kw):
    """the float64 specification with its margins asserted: the input decides nothing within 1e-5 of a tie"""
    loss, dnet, m = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float64, return_margins=True,
                                             **kw)
    assert m["best_thresh"] >= MARGIN and m["shape_gap"] >= MARGIN and m["cell_edge"] >= MARGIN, m
    return loss, dnet


def checked_stats(net, truth, ntruth, anchors, size, tree):
    stats, m = W.region_stats_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float64, return_margins=True)
    assert m["iou_half"] >= MARGIN and m["shape_gap"] >= MARGIN and m["cell_edge"] >= MARGIN, m
    return stats


def owners(truth, ntruth, anchors, size, S):
    """[(image, row, col, anchor, class, truth index)] of the truths that own their slot: the lowest truth index wins"""
    from tensorflow_yolo2_amd.utils.region_loss import shape_ious
    an = np.asarray(anchors, np.float64)
    out, taken = [], set()
    for i in range(len(ntruth)):
        for k in range(int(ntruth[i])):
            t = np.asarray(truth[i, k], np.float64)
            gx, gy, gw, gh = t[0] / size * S, t[1] / size * S, t[2] / size * S, t[3] / size * S
            slot = (i, min(int(gy), S - 1), min(int(gx), S - 1), int(np.argmax(shape_ious(gw, gh, an))))
            if slot not in taken:
                taken.add(slot)
                out.append(slot + (int(t[4]), k))
    return out


GUARD = 1024                        # words behind a gradient buffer that a launch must leave alone


def check_tree_loss_on_the_device(inputs):
    """engine.yolov2_loss_boxes_tree on one parity input (parity_input's tuple) against the float64 specification: default
    and NONDEFAULT scales, forward only, two calls, zero gradients where the specification has zero, a NaN-filled
    gradient buffer with a guard behind it, rows beyond ntruth, class indices outside the tree.  Needs the GPU; prints
    each figure before it asserts.  Gates: loss rtol 2e-5, largest gradient error / largest gradient < 2e-5"""
    import ctypes
    import torch
    from tensorflow_yolo2_amd import _lib, engine as E
    net, truth, ntruth, anchors, size, tree = inputs
    dev = lambda a: torch.as_tensor(np.array(a)).cuda()
    bits = lambda t: t.cpu().numpy().view(np.uint32)

    def assert_close(loss, dnet, ref_loss, ref_d):
        err = np.abs(dnet - ref_d).max() / np.abs(ref_d).max()
        print("loss", loss, "reference", ref_loss, "largest relative error %.3e" % (np.abs(loss - ref_loss) / np.abs(ref_loss)).max())
        print("largest gradient error / largest gradient %.3e" % err)
        np.testing.assert_allclose(loss, ref_loss, rtol=2e-5)
        assert err < 2e-5, err

    n = net.shape[0]
    assert ntruth[0] == 30 and len({(int(t[1] // 32), int(t[0] // 32)) for t in truth[0]}) < 15   # several truths per cell
    tt = E.WordTreeTables(tree)
    nd, cd = dev(net), dev(ntruth)
    args = lambda tr=truth: (nd, dev(tr), cd, anchors, size, tt)
    # default scales
    ref_loss, ref_d = checked_loss(net, truth, ntruth, anchors, size, tree)
    loss, dnet = E.yolov2_loss_boxes_tree(*args())
    assert tuple(dnet.shape) == net.shape
    assert_close(loss.cpu().numpy(), dnet.cpu().numpy(), ref_loss, ref_d)
    assert not dnet.cpu().numpy()[ref_d == 0].any()                      # off the paths and in un-owned rows: exactly 0
    # two calls on the same input: the same bits
    loss_b, dnet_b = E.yolov2_loss_boxes_tree(*args())
    assert np.array_equal(bits(loss), bits(loss_b)) and np.array_equal(bits(dnet), bits(dnet_b))
    del dnet_b
    # a NaN-filled gradient buffer with a guard behind it: every word of every workgroup's span is written, none behind
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    buf = torch.full((net.size + GUARD,), float("nan"), device="cuda")
    guard = dev(np.random.default_rng(n).integers(-2 ** 31, 2 ** 31, GUARD).astype(np.int32))
    buf[net.size:].view(torch.int32).copy_(guard)
    S, B = net.shape[1], net.shape[3]
    ws = torch.empty(lib.y2_yolov2_loss_boxes_tree_workspace_bytes(n, S, B), dtype=torch.uint8, device="cuda")
    loss_c = torch.full((5,), float("nan"), device="cuda")
    ad = dev(np.asarray(anchors, np.float32))
    assert lib.y2_yolov2_loss_boxes_tree(p(nd), p(dev(truth)), p(cd), p(ad), p(tt.tables), n, S, B, tree.n, tt.groups,
                                         tt.max_depth, truth.shape[1], float(size), None, p(loss_c), p(buf), p(ws),
                                         None) == 0, lib.y2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[net.size:].view(torch.int32), guard)
    assert torch.isfinite(buf[:net.size]).all()
    assert np.array_equal(bits(buf[:net.size]), bits(dnet).ravel()) and np.array_equal(bits(loss_c), bits(loss))
    del buf
    # other scales, the area weight and the prior
    ref2, refd2 = checked_loss(net, truth, ntruth, anchors, size, tree, area_weight=True, prior_scale=0.01, **NONDEFAULT)
    sc = dict(NONDEFAULT, area_weight=1.0, prior_scale=0.01)
    l2, d2 = E.yolov2_loss_boxes_tree(*args(), scales=sc)
    assert_close(l2.cpu().numpy(), d2.cpu().numpy(), ref2, refd2)
    assert (np.abs(ref2 - ref_loss) > 1e-3 * np.abs(ref_loss)).all()     # (the scale set changed every part)
    del d2
    # forward only
    l3, d3 = E.yolov2_loss_boxes_tree(*args(), need_grad=False, scales=sc)
    assert d3 is None and np.array_equal(bits(l3), bits(l2))
    # rows beyond ntruth are not read
    dirty = truth.copy()
    for i in range(n):
        dirty[i, ntruth[i]:] = 123.0
    l4, _ = E.yolov2_loss_boxes_tree(*args(dirty), need_grad=False)
    assert np.array_equal(bits(l4), bits(loss))
    # a class index outside [0, C): the row keeps its other terms and takes no class term, its class gradient is zero
    own = owners(truth, ntruth, anchors, size, net.shape[1])
    i, r, q, b, _k, k0 = own[0]
    for value in (float(tree.n), -1.0):
        bad = truth.copy()
        bad[i, k0, 4] = value
        r_bad, rd_bad = checked_loss(net, bad, ntruth, anchors, size, tree)
        l_bad, d_bad = E.yolov2_loss_boxes_tree(*args(bad))
        assert_close(l_bad.cpu().numpy(), d_bad.cpu().numpy(), r_bad, rd_bad)
        assert not d_bad.cpu().numpy()[i, r, q, b, 5:].any() and d_bad.cpu().numpy()[i, r, q, b, :5].all()
        assert r_bad[3] < ref_loss[3] and np.array_equal(bits(l_bad)[:3], bits(loss)[:3])


def check_tree_stats_on_the_device(inputs):
    """engine.yolov2_region_stats_tree on one parity input against the float64 specification: rtol 2e-5 on the four means,
    recall and count exact, two runs the same bits, everything but the class statistic the flat entry's bits"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, truth, ntruth, anchors, size, tree = inputs
    dev = lambda a: torch.as_tensor(np.array(a)).cuda()
    tt = E.WordTreeTables(tree)
    ref = checked_stats(net, truth, ntruth, anchors, size, tree)
    out = torch.full((6,), float("nan"), device="cuda")
    nd, td, cd = dev(net), dev(truth), dev(ntruth)
    got = E.yolov2_region_stats_tree(nd, td, cd, anchors, size, tt, out=out)
    assert got is out
    stats = out.cpu().numpy()
    print("stats", stats, "reference", ref, "largest relative error %.3e" % (np.abs(stats[:4] - ref[:4]) / np.abs(ref[:4])).max())
    np.testing.assert_allclose(stats[:4], ref[:4], rtol=2e-5)
    assert stats[4] == np.float32(ref[4]) and stats[5] == ref[5] == ntruth.sum()
    again = E.yolov2_region_stats_tree(nd, td, cd, anchors, size, tt).cpu().numpy()
    assert again.tobytes() == stats.tobytes()                            # two runs: the same bits
    flat = E.yolov2_region_stats(nd, td, cd, anchors, size).cpu().numpy()
    assert np.delete(flat, 1).tobytes() == np.delete(stats, 1).tobytes() and flat[1] != stats[1]


HEAD_ROWS = 203                     # not a multiple of the four rows of a workgroup
HEAD_SEEDS = {"small": 5, "wide": 6}


def head_input(name):
    """(net [HEAD_ROWS][5 + C] float32, tree): class logits spread widely enough that walks stop at every level"""
    tree = small_tree() if name == "small" else wide_tree()
    rng = np.random.default_rng(HEAD_SEEDS[name])
    net = (rng.standard_normal((HEAD_ROWS, 5 + tree.n)) * 2.0).astype(np.float32)
    return net, tree
