"""The inputs of tests/test_gpu_yolo9000_width.py on the host (no GPU): every condition those tests rely on is asserted
here, on the float64 specification, so that none of it is assumed on the device -- the tree's shape, the depths and groups
the head rows reach, the margins and owned slots of the loss input, the room the float32 specification leaves under the GPU
gates at rows of 9,423 floats, and the share of f16 subnormals among the GEMM operands."""
import numpy as np
import pytest

import _word_tree_cases as WT
import _yolo9000_cases as Y
from tensorflow_yolo2_amd.utils import word_tree as W

MARGIN = WT.MARGIN


def test_big_tree_has_the_shape_the_kernels_are_tested_on():
    t = Y.big_tree()
    assert t.n == 9418 == Y.NODES and t.max_depth == 14 and (t.parent < 0).sum() == 9
    assert {1, 2, 37, 63, 64, 65, 129, 1025} <= set(t.group_size.tolist()) and t.group_size.max() == 1025
    assert len(t.group_offset) == 238 and len(W.pack(t)) == 28730 and (5 + t.n) % 2 == 1
    assert 5 + t.n > 256                                                  # a row is longer than a workgroup's stride
    for parent, size in Y.SPECIAL:
        off, _ = Y.group_of(t, size)
        assert t.parent[off] == parent and t.parent[off + size - 1] == parent
    # the chain: every depth 2..14 holds a leaf and, down to 13, the parent of the next group of two
    last = Y.group_of(t, 1025)[0] + 1024
    for depth in range(2, 15):
        leaf = Y.chain_leaf(t, depth)
        assert t.parent[leaf] == last and t.parent[leaf + 1] == last
        last = leaf + 1
    assert W.path_to_root(t, Y.chain_leaf(t, 14))[-1] == 0 and len(W.path_to_root(t, Y.chain_leaf(t, 14))) == 15


def test_head_rows_stop_at_every_depth_and_in_every_special_group():
    net, tree = Y.head_rows()
    assert net.shape == (203, 9423) and net.shape[0] % 4
    random_only = W.word_tree_head(net[len(Y.planted_nodes(tree)):], tree, Y.DEPTH_THRESH)[1]
    assert tree.depth[random_only].max() <= 2                             # what the planted rows are there for
    for thresh in Y.HEAD_THRESHOLDS:
        _out, top, prob, m = W.word_tree_head(net, tree, thresh, return_margins=True)
        assert m["thresh"] >= MARGIN and m["group_gap"] >= MARGIN, (thresh, m)
        depths = set(tree.depth[top].tolist())
        sizes = set(tree.group_size[tree.group[top]].tolist())
        print("thresh %.1f: margins %s, depths %s, group sizes %s, least prob %.3e" % (thresh, m, sorted(depths),
                                                                                     sorted(sizes), prob.min()))
        if thresh == Y.DEPTH_THRESH:
            assert depths == set(range(15))
            assert {1, 2, 63, 64, 65, 129, 1025} <= sizes
        if thresh == 0.0:                                                 # every walk ends in a leaf; no root is one
            assert (tree.child[top] < 0).all() and depths == set(range(1, 15))
            planted = np.asarray(Y.planted_nodes(tree))
            leaves = tree.child[planted] < 0
            assert np.array_equal(top[:len(planted)][leaves], planted[leaves]) and leaves.sum() == 18


@pytest.mark.parametrize("key", sorted(Y.SHAPES))
def test_loss_input_decides_nothing_near_a_tie_and_owns_slots_in_both_workgroups(key):
    net, truth, ntruth, anchors, size, tree = Y.parity_input(key)
    assert net.shape == (2, 10, 10, 3, 5 + tree.n) and ntruth.tolist() == [30, 5]
    assert 256 < net.shape[1] * net.shape[2] * net.shape[3] == 300        # two workgroups, the second with 44 live slots
    for kw in ({}, dict(area_weight=True, prior_scale=0.01, **WT.NONDEFAULT)):
        _loss, _d, m = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, tree, return_margins=True, **kw)
        print(key, kw, m)
        assert m["best_thresh"] >= MARGIN and m["shape_gap"] >= MARGIN and m["cell_edge"] >= MARGIN, m
    _stats, m = W.region_stats_boxes_tree(net, truth, ntruth, anchors, size, tree, return_margins=True)
    print(key, "statistics", m)
    assert m["iou_half"] >= MARGIN and m["shape_gap"] >= MARGIN and m["cell_edge"] >= MARGIN, m
    own = WT.owners(truth, ntruth, anchors, size, Y.S)
    slots = [(r * Y.S + q) * 3 + b for (_i, r, q, b, _c, _k) in own]
    assert min(slots) < 256 <= max(slots) and sum(s >= 256 for s in slots) >= 4
    # every placed class owns a slot: truths 0..8 of image 0, shadowed by no lower index
    placed = Y.placed_classes(tree)
    assert [(k, c) for (i, _r, _q, _b, c, k) in own if i == 0 and k < len(placed)] == list(enumerate(placed))
    assert len(set(placed)) == len(placed)
    assert {(int(t[1] // 32), int(t[0] // 32)) for t in truth[0, :len(placed)]} == set(Y.PLACED_CELLS)
    if key == "n2_S10_B3_big":
        assert tree.depth[placed[0]] == 14 and tree.parent[placed[4]] < 0
        assert [int(tree.group_size[tree.group[c]]) for c in placed] == [2, 1025, 1025, 1, 9, 63, 64, 65, 129]
    else:
        assert 5 + tree.n == 75 and 256 % 75


@pytest.mark.parametrize("key", sorted(Y.SHAPES))
def test_float32_specification_stays_far_inside_the_gpu_gates(key):
    """the GPU gates are 2e-5; the specification's own float32 arithmetic differs from float64 by at most 2e-6 here"""
    net, truth, ntruth, anchors, size, tree = Y.parity_input(key)
    l64, d64 = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float64)
    l32, d32 = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float32)
    loss_err = (np.abs(l32 - l64) / np.abs(l64)).max()
    grad_err = np.abs(d32 - d64).max() / np.abs(d64).max()
    s64 = W.region_stats_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float64)
    s32 = W.region_stats_boxes_tree(net, truth, ntruth, anchors, size, tree, dtype=np.float32)
    assert np.float32(s64[4]) == s32[4] and s64[5] == s32[5] == 35          # recall and count: the same decisions
    stats_err = (np.abs(s32[:4] - s64[:4]) / np.abs(s64[:4])).max()
    print("%s float32 against float64: loss %.3e, gradient %.3e, statistics %.3e" % (key, loss_err, grad_err, stats_err))
    assert loss_err <= 2e-6 and grad_err <= 2e-6 and stats_err <= 2e-6


def test_subnormal_gemm_operands_are_mostly_f16_subnormals():
    x, Wt, b = Y.gemm_operands_subnormal(*Y.SUBNORMAL_SHAPE)
    assert x.shape == (147, 128) and Wt.shape == (128, 225) and not b.any()
    print("nonzero f16 subnormals: x %.3f, W %.3f" % (Y.subnormal_share(x), Y.subnormal_share(Wt)))
    assert Y.subnormal_share(x) >= 0.5 and Y.subnormal_share(Wt) >= 0.5
    # the products are far inside fp32's normal range: only the f16 side of the kernel meets subnormals
    ref, mag = Y.WH.gemm_reference(x, Wt, b)
    assert (np.abs(ref) > 1e-25).mean() > 0.95
    # ... and nearly every sum stands far above the GEMM gate's bound: there a kernel that flushed would return 0 and fail
    assert (np.abs(ref) > 100.0 * (2.0 * 128 * 2.0 ** -24 * mag + 1e-30)).mean() > 0.9


def test_yolo9000_width_cfg_is_chain_wide_with_the_real_head(tmp_path):
    from tensorflow_yolo2_amd.utils import darknet_cfg as C
    record = C.load(Y.write_yolo9000_width_files(tmp_path), wide_head=True)
    assert record.classes == 9418 and record.num == 3 and record.tree == "big.tree" and record.tree_thresh == 0.4
    graph = C.compile_graph(record, wide_head=True)
    assert graph.wide is True and graph.file_layers[-1] == (1, 128, 28269, False)
