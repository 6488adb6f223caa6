"""Inputs shared by tests/test_detect_tree_host.py and tests/test_gpu_detect_tree.py: the heads of
tests/test_gpu_detect_anchor.py's _anchor_case (the hand-made candidates, an image with nothing above the threshold, an
image that overflows max_out) on a word tree, with the class logits of the named candidates planted along tree paths so
that `a` and `a_same` land on one node and `a_other` on another.  Everything is generated on the CPU from fixed seeds."""
import numpy as np

import _word_tree_cases as WT
import _yolo9000_cases as Y
from test_gpu_detect_anchor import ANCHORS, _anchor_case
from tensorflow_yolo2_amd.utils import word_tree as W

TREE_THRESH = 0.5
BOOST = 12.0                        # exp(12) against a group of zeros: every conditional on a planted path is > 0.99


TREES = {"small": WT.small_tree, "wide70": WT.wide_tree, "big": Y.big_tree}      # 20, 70 and 9,418 nodes


def planted_nodes(tree):
    """(the node of a / a_same, the node of a_other, the node of every other named candidate): two leaves and a root"""
    leaves = np.nonzero(np.asarray(tree.child) < 0)[0]
    return int(leaves[-1]), int(leaves[len(leaves) // 2]), 0


def tree_case(S, B, tree):
    """_anchor_case(S, B, tree.n) -> (net [3][S][S][B][5 + C], named, {name: planted node}): the named candidates' class
    logits are zero but for BOOST along the path of their node, so the walk ends there at any tree_thresh below 0.9; the
    six `run` candidates keep their (copied, equal) random logits and the other rows their random ones"""
    net, named = _anchor_case(S, B, tree.n)
    node_a, node_other, node_rest = planted_nodes(tree)
    assert node_a != node_other
    rows = net[0].reshape(S * S * B, 5 + tree.n)
    nodes = {}
    for name, i in named.items():
        if name.startswith("run"):
            continue
        node = node_a if name in ("a", "a_same") else node_other if name == "a_other" else node_rest
        rows[i, 5:] = 0.0
        for a in W.path_to_root(tree, node):
            rows[i, 5 + a] = np.float32(BOOST)
        nodes[name] = node
    return net, named, nodes


def host_decode(net, tree, tree_thresh=TREE_THRESH):
    """the oracle's float32 decode of the head the host walk rewrote -> (boxes [n][K][4], so [n][K], top [n][K]): what
    the device hands the specification in the GPU tests, from the CPU alone"""
    from oracle import ext_ref as X
    n, S, _, B, D = net.shape
    out, top, _prob = W.word_tree_head(net.reshape(-1, D), tree, tree_thresh)
    boxes, scores = X.decode_anchors(out.reshape(net.shape), ANCHORS[:B])
    scores = scores.reshape(-1, D - 5)
    so = scores[np.arange(len(top)), top]
    return boxes, so.reshape(n, -1), top.reshape(n, -1)


def one_hot(so, top, C):
    """scores [K][C]: so at top, zero elsewhere -- what y2_decode_anchors makes of a rewritten row"""
    scores = np.zeros((len(so), C), np.float32)
    scores[np.arange(len(so)), top] = so
    return scores

