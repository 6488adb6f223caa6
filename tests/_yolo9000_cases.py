"""Inputs at YOLO9000's real width, shared by tests/test_yolo9000_cases_host.py and tests/test_gpu_yolo9000_width.py: a
9,418-node tree (rows of 9,423 floats), head rows whose walks stop at every depth 0..14, a two-workgroup loss / statistics
input on that tree, GEMM operands in f16's subnormal range and the cfg of a detector with 28,269 filters.  Everything is
generated on the CPU from fixed seeds; the host file asserts every condition the GPU tests rely on (margins, depths reached,
slots owned on both sides of slot 256, the share of subnormal operands)."""
import os

import numpy as np

import _wide_head_cases as WH
import _word_tree_cases as WT
from tensorflow_yolo2_amd.utils import word_tree as W

NODES, ROOTS, MAX_DEPTH = 9418, 9, 14
# (parent, size) of the special groups in file order; their first node follows from the sizes: 9, 1034, 1098, 1161, 1226, 1355
SPECIAL = ((0, 1025), (1, 64), (2, 63), (3, 65), (4, 129), (5, 1))
FILL = 37


def big_tree_text():
    """9,418 nodes, 238 groups: 9 roots; under roots 0..5 groups of 1025 (16 lane strides + 1), 64, 63, 65, 129 and 1; a
    chain of groups of 2 from the last member of the 1025-group (depth 1) down to depth 14, each under the last member of
    the group above; the remaining 8,036 nodes in groups of 37 (the last one holds 7) under consecutive parents: roots 6..8,
    then the members of the 1025-group from its first.  It mirrors what makes YOLO9000's tree hard, not its labels"""
    lines = ["root%d -1" % i for i in range(ROOTS)]
    for parent, size in SPECIAL:
        lines += ["g%d_%d %d" % (size, i, parent) for i in range(size)]
    at = ROOTS + SPECIAL[0][1] - 1                                        # the last member of the 1025-group
    for depth in range(2, MAX_DEPTH + 1):
        lines += ["chain%d_%d %d" % (depth, i, at) for i in range(2)]
        at = len(lines) - 1
    parent = 6
    while len(lines) < NODES:
        lines += ["f%d_%d %d" % (parent, i, parent) for i in range(min(FILL, NODES - len(lines)))]
        parent += 1
    return "\n".join(lines) + "\n"


_TREE = []


def big_tree():
    if not _TREE:
        _TREE.append(W.parse(big_tree_text(), "<big>"))
    return _TREE[0]


def group_of(tree, size):
    """-> (first node, size) of the one group of that size among SPECIAL"""
    (g,) = np.nonzero(tree.group_size == size)[0]
    return int(tree.group_offset[g]), size


def chain_leaf(tree, depth):
    """the first member (a leaf) of the chain's group at depth 2..14"""
    off = ROOTS + sum(s for _p, s in SPECIAL) + 2 * (depth - 2)
    assert tree.depth[off] == depth and tree.child[off] < 0 and tree.group_size[tree.group[off]] == 2
    return off


# ---- head rows
HEAD_ROWS, HEAD_SEED, HEAD_BOOST = 203, 44, 12.0
HEAD_THRESHOLDS = (0.0, 0.3, 0.9)
DEPTH_THRESH = 0.3                  # the threshold at which the planted rows stop at every depth 0..14


def planted_nodes(tree):
    """the nodes whose paths carry HEAD_BOOST in rows 0, 1, ...: root 0 (its 1025 children are not convincing: depth 0); a
    childless member of the 1025-group (depth 1); the chain's leaf of each depth 2..14; then the last member of the 64-,
    63-, 65- and 129-groups, the first of the 1025-group and root 5, whose group of one the walk always enters"""
    o1025 = group_of(tree, 1025)[0]
    nodes = [0, o1025 + 700] + [chain_leaf(tree, d) for d in range(2, MAX_DEPTH + 1)]
    nodes += [sum(group_of(tree, s)) - 1 for s in (64, 63, 65, 129)] + [o1025, 5]
    return nodes


_HEAD = []


def head_rows():
    """(net [203][9423] float32, tree): standard_normal * 2, which alone never walks deeper than 2; the first rows carry
    HEAD_BOOST along the paths of planted_nodes"""
    if not _HEAD:
        tree = big_tree()
        rng = np.random.default_rng(HEAD_SEED)
        net = (rng.standard_normal((HEAD_ROWS, 5 + tree.n)) * 2.0).astype(np.float32)
        for row, node in enumerate(planted_nodes(tree)):
            for a in W.path_to_root(tree, node):
                net[row, 5 + a] += np.float32(HEAD_BOOST)
        net.setflags(write=False)
        _HEAD.append((net, tree))
    return _HEAD[0]


# ---- loss and statistics
# key -> (tree, seed); both: n = 2, S = 10, anchors THREE: 300 slots, two workgroups, the second with 44 live slots
SHAPES = {"n2_S10_B3_big": (big_tree, 7), "n2_S10_B3_wide": (WT.wide_tree, 7)}
N, S = 2, 10
# the cells (row, col) of the placed truths of image 0, one each: slots 3 (r S + q) + anchor on both sides of slot 256
PLACED_CELLS = ((0, 1), (9, 8), (2, 3), (8, 7), (4, 5), (9, 2), (5, 0), (8, 9), (3, 6))


def placed_classes(tree):
    """the truth classes that are placed, not drawn (the big tree; on another tree: its last node, first node and roots):
    the depth-14 leaf; the first and last member of the 1025-group; the group-of-one member; a root; a member each of the
    63-, 64-, 65- and 129-groups"""
    if tree.n != NODES:
        return [tree.n - 1, 0] + [int(k) for k in np.nonzero(tree.depth == 1)[0][:7]]
    o1025 = group_of(tree, 1025)[0]
    return [chain_leaf(tree, MAX_DEPTH), o1025, o1025 + 1024, group_of(tree, 1)[0], 7, group_of(tree, 63)[0] + 62,
            group_of(tree, 64)[0] + 63, group_of(tree, 65)[0] + 64, group_of(tree, 129)[0] + 128]


_PARITY = {}


def parity_input(key):
    """(net, truth [2][30][5], ntruth = (30, 5), anchors, size, tree) as tests/_word_tree_cases.py parity_input gives it.
    Image 0: truths 0..8 carry placed_classes in PLACED_CELLS (the lowest indices: no other truth shadows them), the other
    21 fall into four hot cells with random classes; image 1: the deepest placed class in the last cell, the next in the
    first, three random truths"""
    if key not in _PARITY:
        make_tree, seed = SHAPES[key]
        tree = make_tree()
        anchors = WT.THREE
        B, C, size = len(anchors), tree.n, 32 * S
        rng = np.random.default_rng(seed)
        net = (rng.standard_normal((N, S, S, B, 5 + C)) * 0.7).astype(np.float32)
        truth = np.zeros((N, 30, 5), np.float32)
        ntruth = np.asarray([30, 5], np.int32)
        an = np.asarray(anchors)
        placed = placed_classes(tree)
        assert len(placed) == len(PLACED_CELLS)
        hot = np.asarray(((1, 1), (6, 4), (9, 5), (9, 9)))                # two of the four in the second workgroup
        for i in range(N):
            k = int(ntruth[i])
            which = rng.integers(0, B, k)
            scale = rng.uniform(0.75, 1.3, (k, 2))
            cell = hot[rng.integers(0, 4, k)] if i == 0 else rng.integers(0, S, (k, 2))
            cls = rng.integers(0, C, k)
            if i == 0:
                cell[:len(placed)], cls[:len(placed)] = PLACED_CELLS, placed
            else:
                cell[:2], cls[:2] = ((S - 1, S - 1), (0, 0)), placed[:2]
            centre = (cell[:, ::-1] + rng.uniform(0.05, 0.95, (k, 2))) * 32.0    # (x, y) from (row, col)
            truth[i, :k, 0:2] = centre
            truth[i, :k, 2:4] = np.minimum(an[which] * scale * 32.0, size - 1.0)
            truth[i, :k, 4] = cls
        for a in (net, truth, ntruth):
            a.setflags(write=False)
        _PARITY[key] = (net, truth, ntruth, anchors, size, tree)
    return _PARITY[key]


# ---- the wide head's GEMM
# (the five shapes of the tile, row-tile, K-tail and K-limit regimes stand in tests/_wide_head_cases.py GEMM_SHAPES)
SUBNORMAL_SHAPE = (147, 128, 225)


def gemm_operands_subnormal(M, K, Cout):
    """tests/_wide_head_cases.py gemm_operands with row m of x scaled by 2^-(16 + m % 7) and W by 2^-12, so that most
    operands are f16 subnormals (below 2^-14) and none is lost entirely.  The bias is zero: the products are of order
    2^-35, one rounding of a bias add of the usual size would exceed the gate's bound, and without it a kernel that
    flushes subnormals returns exactly 0"""
    x, Wt, b = WH.gemm_operands(M, K, Cout)
    x = x * np.exp2(-(16.0 + np.arange(M) % 7)).astype(np.float32)[:, None]
    return x, Wt * np.float32(2.0 ** -12), np.zeros_like(b)


def subnormal_share(a):
    """the share of a's elements that are nonzero f16 subnormals once rounded to f16"""
    h = np.abs(a.astype(np.float16).astype(np.float64))
    return float(((h > 0) & (h < 2.0 ** -14)).mean())


# ---- the detector at 28,269 filters
def write_yolo9000_width_files(tmp_path):
    """chain-wide.cfg with filters=28269, classes=9418 and tree=big.tree, and that tree, in tmp_path -> the cfg's path"""
    tmp_path = str(tmp_path)
    with open(WH.CHAIN_WIDE_CFG) as f:
        text = f.read()
    for old, new in (("filters=2115\n", "filters=%d\n" % WH.YOLO9000_FILTERS), ("classes=700\n", "classes=%d\n" % NODES),
                     ("tree=wide700.tree\n", "tree=big.tree\n")):
        assert text.count(old) == 1, old
        text = text.replace(old, new)
    cfg = os.path.join(tmp_path, "chain-9000.cfg")
    with open(cfg, "w") as f:
        f.write(text)
    with open(os.path.join(tmp_path, "big.tree"), "w") as f:
        f.write(big_tree_text())
    return cfg


# the file's tree_thresh and the weights seed under which the detector's walks reach more than 10 distinct nodes
DETECTOR_TREE_THRESH, DETECTOR_WEIGHTS_SEED = 0.4, 21
