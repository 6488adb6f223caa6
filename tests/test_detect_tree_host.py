"""Host tests (no GPU) of the word-tree detect path's specification: utils/detect_batch.anchor_detect_tree_darknet against
anchor_detect_classes_darknet on the scores a rewritten head decodes to (one-hot objectness at the node), its cap, the
proof that the inputs of tests/test_gpu_detect_tree.py exercise every rule, and evaluate_yolov2's tree_rows argument."""
import types

import numpy as np
import pytest

import _detect_tree_cases as T
from test_gpu_detect_anchor import SHAPES
from tensorflow_yolo2_amd.utils import detect_batch as DB

SCORE_THRESH, IOU_THRESH, MAX_OUT = 0.2, 0.45, 24
GEOMETRIES = ((5, 5, "small"), (13, 5, "wide70"))

_CASES = {}


def _case(S, B, name):
    """(tree, named, nodes, boxes, so, top) of one geometry, decoded once and shared"""
    if (S, B, name) not in _CASES:
        tree = T.TREES[name]()
        net, named, nodes = T.tree_case(S, B, tree)
        _CASES[S, B, name] = (tree, named, nodes) + T.host_decode(net, tree)
    return _CASES[S, B, name]


@pytest.mark.parametrize("S,B,name", GEOMETRIES)
def test_flat_tree_rows_are_the_per_class_segments_of_the_one_hot_scores(S, B, name):
    tree, _named, _nodes, boxes, so, top = _case(S, B, name)
    K, C, N = S * S * B, tree.n, 32 * S
    assert K not in (64, 128, 256, 512, 1024, 2048)
    for img, score_thresh, iou_thresh in ((0, SCORE_THRESH, IOU_THRESH), (2, SCORE_THRESH, IOU_THRESH), (0, 0.0, 0.0),
                                          (2, 0.005, 1.0), (1, SCORE_THRESH, IOU_THRESH)):
        h, w = SHAPES[img]
        det, score = DB.anchor_detect_tree_darknet(boxes[img], so[img], top[img], w, h, score_thresh, iou_thresh, K, N)
        want = DB.anchor_detect_classes_darknet(boxes[img], T.one_hot(so[img], top[img], C), w, h, score_thresh, iou_thresh,
                                                K, N)
        assert len(det) == want[2].sum()
        assert (np.diff(score.astype(np.float64)) <= 0).all()              # one descending order per image
        ties = np.nonzero(np.diff(score.astype(np.float64)) == 0)[0]
        assert (det[ties, 5] < det[ties + 1, 5]).all()                     # ties by ascending candidate
        for c in range(C):
            sel = det[:, 4] == c
            cnt = int(want[2][c])
            assert sel.sum() == cnt, (img, c)
            assert np.array_equal(det[sel], want[0][c, :cnt]), (img, c)
            assert np.array_equal(score[sel].view(np.uint32), want[1][c, :cnt].view(np.uint32)), (img, c)
        assert img != 1 or len(det) == 0                                   # nothing above the threshold


@pytest.mark.parametrize("S,B,name", GEOMETRIES)
def test_a_binding_max_out_keeps_the_first_rows_of_the_uncapped_run(S, B, name):
    tree, _named, _nodes, boxes, so, top = _case(S, B, name)
    K, N = S * S * B, 32 * S
    h, w = SHAPES[2]
    full = DB.anchor_detect_tree_darknet(boxes[2], so[2], top[2], w, h, SCORE_THRESH, IOU_THRESH, K, N)
    assert len(full[0]) > MAX_OUT                                          # the image overflows the small cap
    for cap in (1, MAX_OUT):
        det, score = DB.anchor_detect_tree_darknet(boxes[2], so[2], top[2], w, h, SCORE_THRESH, IOU_THRESH, cap, N)
        assert len(det) == cap and np.array_equal(det, full[0][:cap])
        assert np.array_equal(score.view(np.uint32), full[1][:cap].view(np.uint32))


@pytest.mark.parametrize("S,B,name", GEOMETRIES)
def test_detect_tree_inputs_exercise_every_rule(S, B, name):
    """with the oracle's float32 decode in front, both specifications keep, suppress within a node and not across nodes,
    drop for every reason, meet equal scores and run out of max_out on the inputs the GPU tests use"""
    tree, named, nodes, boxes, so, top = _case(S, B, name)
    K, N = S * S * B, 32 * S
    h, w = SHAPES[0]
    for cand, node in nodes.items():
        assert top[0][named[cand]] == node, cand                           # the planted paths are walked to their end
    assert top[0][named["a"]] == top[0][named["a_same"]] != top[0][named["a_other"]]
    assert len(set(top[0].tolist())) > 3 and len(set(top[2].tolist())) > 3  # top takes several nodes
    runs = [named["run%d" % k] for k in range(6)]
    assert len({so[0][i].tobytes() for i in runs}) == 1 and len({int(top[0][i]) for i in runs}) == 1
    assert np.isnan(so[0][named["nan_to"]]) and np.isinf(boxes[0][named["inf_width"], 2])
    # the integer rows: anchor_detect(boxes, so, top, ...) as it stands
    valid, _box, _cls, _score = DB.anchor_candidates(boxes[0], so[0], top[0], w, h, SCORE_THRESH)
    for cand in ("nan_to", "inf_width", "huge_height", "no_width"):
        assert not valid[named[cand]], cand
    for net_size in (None, N):
        det, _s = DB.anchor_detect(boxes[0], so[0], top[0], w, h, SCORE_THRESH, IOU_THRESH, K, net_size=net_size)
        kept = det[:, 5].tolist()
        assert 0 < len(kept) < valid.sum()
        assert named["a"] in kept and named["a_same"] not in kept and named["a_other"] in kept, net_size
        assert len([i for i in kept if i in runs]) > 1
        counts = [len(DB.anchor_detect(boxes[k], so[k], top[k], SHAPES[k][1], SHAPES[k][0], SCORE_THRESH, IOU_THRESH,
                                       MAX_OUT, net_size=net_size)[0]) for k in range(3)]
        assert counts[1] == 0 and counts[2] == MAX_OUT and 0 < counts[0]
    # a_same falls to a because they share a node: on a node of its own it is kept
    other = top[0].copy()
    other[named["a_same"]] = nodes["left_top"]                             # a node whose other boxes are far away
    assert nodes["left_top"] not in (nodes["a"], nodes["a_other"])
    assert named["a_same"] in DB.anchor_detect(boxes[0], so[0], other, w, h, SCORE_THRESH, IOU_THRESH, K)[0][:, 5].tolist()
    # Darknet's rows: the same keeps; a finite box beyond 2^30 and an empty box are valid there, a NaN and an inf are not
    det, _s = DB.anchor_detect_tree_darknet(boxes[0], so[0], top[0], w, h, SCORE_THRESH, IOU_THRESH, K, N)
    kept = det[:, 5].tolist()
    assert named["a"] in kept and named["a_same"] not in kept and named["a_other"] in kept
    assert named["huge_height"] in kept and named["no_width"] in kept
    assert named["nan_to"] not in kept and named["inf_width"] not in kept
    assert [i for i in kept if i in runs] == sorted(i for i in kept if i in runs) and len([i for i in kept if i in runs]) > 1
    # a skipped row's -1 is not valid
    skipped = top[0].copy()
    skipped[named["a"]] = -1
    kept = DB.anchor_detect_tree_darknet(boxes[0], so[0], skipped, w, h, SCORE_THRESH, IOU_THRESH, K, N)[0][:, 5].tolist()
    assert named["a"] not in kept and named["a_same"] in kept


def test_evaluate_yolov2_checks_tree_rows_before_anything_runs():
    from tensorflow_yolo2_amd.pascal.pascal_eval_yolov2 import evaluate_yolov2
    imdb = types.SimpleNamespace(batch_size=2, entries=[])
    flat = types.SimpleNamespace(tree=None, wide=None, topology="darknet", batch=2, size=64)
    with pytest.raises(ValueError, match="tree_rows=True needs a detector with a word tree"):
        evaluate_yolov2(flat, imdb, 64, per_class=True, tree_rows=True)
    wide_without_tree = types.SimpleNamespace(tree=None, wide=object(), topology="darknet", batch=2, size=64)
    with pytest.raises(ValueError, match="tree_rows=True needs a detector with a word tree"):
        evaluate_yolov2(wide_without_tree, imdb, 64, per_class=True)        # None: the detector has a wide head
    tree = types.SimpleNamespace(tree=object(), wide=None, topology="paper", batch=2, size=64)
    with pytest.raises(ValueError, match="neither 'repo' nor 'darknet'"):
        evaluate_yolov2(tree, imdb, 64, protocol="other", tree_rows=True)
    with pytest.raises(ValueError, match="per_class=True"):
        evaluate_yolov2(tree, imdb, 64, protocol="darknet", tree_rows=True)  # the protocol's own conditions still hold
    with pytest.raises(ValueError, match="\"darknet\" topology"):
        evaluate_yolov2(tree, imdb, 64, per_class=True, letterbox=True, protocol="darknet", tree_rows=True)
