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


HEAD_ROWS = 203                     # not a multiple of the four rows of a workgroup
HEAD_SEEDS = {"small": 5, "wide": 6}


def head_input(name):
    """(net [HEAD_ROWS][5 + C] float32, tree): class logits spread widely enough that walks stop at every level"""
    tree = small_tree() if name == "small" else wide_tree()
    rng = np.random.default_rng(HEAD_SEEDS[name])
    net = (rng.standard_normal((HEAD_ROWS, 5 + tree.n)) * 2.0).astype(np.float32)
    return net, tree
