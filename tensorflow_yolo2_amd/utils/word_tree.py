"""The word tree of the region layer (YOLO9000's `softmax_tree`), as a host specification (numpy only): the tree file, the
record it becomes, the int32 tables the kernels read, the hierarchical probabilities, the loss, the statistics and the
rewritten detection head.  Written from the semantics of Darknet's tree.c and region_layer.c; where this file and
Darknet differ ("The word tree") this file is what csrc/word_tree.hip is tested against.

Tree file.  One node per non-empty line, `label parent`, separated by whitespace; `parent` is a node index, -1 a root;
nodes are numbered from 0 in file order.  A parent's index is below its child's, the roots come first and the nodes of
one parent are consecutive: such a run is a GROUP, and groups are numbered in the order of their first node (group 0 =
the roots).  Anything else is refused with file:line and the item.

Probabilities.  cond = a softmax within each group; abs[i] = cond[i] for a root, else abs[parent[i]] * cond[i].  The
prediction of a row walks DOWN from the root group, taking the first maximum of each group, while the product of the
conditionals stays above the threshold (top_prediction).

pack().  One int32 array of 3 n + 2 G entries: parent[n], group[n], child[n], group_offset[G], group_size[G], in that
order (TABLE_* below name the segments).  n, G and max_depth travel next to it as plain integers."""
import collections

import numpy as np

from .region_loss import _box_iou_cwh, shape_ious

# n: node count; labels: the first word of each line; parent / group / child / depth: int64 [n] (child: the group whose
# members have this node as parent, -1 for a leaf); group_offset / group_size: int64 [G]; max_depth: the largest depth
WordTree = collections.namedtuple("WordTree", "path n labels parent group group_offset group_size child depth max_depth")

TABLE_SEGMENTS = ("parent", "group", "child", "group_offset", "group_size")


def _fail(path, line, what):
    raise ValueError("%s:%d: %s" % (path, line, what))


def parse(text, path="<tree>"):
    """the text of a tree file -> WordTree; `path` is the name the errors carry"""
    labels, parent, lines = [], [], []
    last = 1
    for no, raw in enumerate(text.splitlines(), 1):
        s = raw.split()
        last = no
        if not s:
            continue
        if len(s) != 2:
            _fail(path, no, "%r is not `label parent`" % raw.strip())
        try:
            p = int(s[1])
        except ValueError:
            _fail(path, no, "parent %r is no integer" % s[1])
        i = len(labels)
        if p < -1:
            _fail(path, no, "node %d: parent %d is neither a node index nor -1" % (i, p))
        if p >= i:
            _fail(path, no, "node %d: parent %d is not below its child" % (i, p))
        labels.append(s[0])
        parent.append(p)
        lines.append(no)
    n = len(labels)
    if n == 0:
        _fail(path, last, "the file holds no node")
    if parent[0] != -1:
        _fail(path, lines[0], "node 0: parent %d: the roots come first" % parent[0])
    group, offsets, sizes = [], [], []
    seen = set()                     # parents whose run has ended or is running
    for i in range(n):
        if i and parent[i] == parent[i - 1]:
            sizes[-1] += 1
        else:
            if parent[i] in seen:
                _fail(path, lines[i], ("node %d: a root behind a child: the roots come first" % i) if parent[i] < 0 else
                      "node %d: the nodes of parent %d are not consecutive" % (i, parent[i]))
            seen.add(parent[i])
            offsets.append(i)
            sizes.append(1)
        group.append(len(offsets) - 1)
    child = [-1] * n
    for g, off in enumerate(offsets):
        if parent[off] >= 0:
            child[parent[off]] = g
    depth = [0] * n
    for i in range(n):
        depth[i] = 0 if parent[i] < 0 else depth[parent[i]] + 1
    a = lambda v: np.asarray(v, np.int64)
    return WordTree(path=path, n=n, labels=tuple(labels), parent=a(parent), group=a(group), group_offset=a(offsets),
                    group_size=a(sizes), child=a(child), depth=a(depth), max_depth=int(max(depth)))


def load(path):
    """a tree file -> WordTree"""
    with open(path, "r") as f:
        return parse(f.read(), str(path))


def flat(n):
    """the tree of n roots: one group, the plain softmax"""
    return parse("".join("c%d -1\n" % i for i in range(n)), "<flat %d>" % n)


def pack(tree):
    """-> int32 [3 n + 2 G]: parent, group, child, group_offset, group_size (the layout csrc/word_tree.hip reads)"""
    return np.concatenate([np.asarray(getattr(tree, k), np.int64) for k in TABLE_SEGMENTS]).astype(np.int32)


def groups(tree):
    return len(tree.group_offset)


def conditional(logits, tree, dtype=np.float64):
    """logits [..., n] -> the softmax within each group, shifted by the group's maximum"""
    lg = np.asarray(logits, dtype)
    assert lg.shape[-1] == tree.n, (lg.shape, tree.n)
    out = np.empty_like(lg)
    for off, size in zip(tree.group_offset, tree.group_size):
        v = lg[..., off:off + size]
        e = np.exp(v - v.max(axis=-1, keepdims=True))
        out[..., off:off + size] = e / e.sum(axis=-1, keepdims=True)
    return out


def absolute(cond, tree):
    """cond [..., n] -> abs: in ascending index, cond[i] for a root, else abs[parent[i]] * cond[i]"""
    out = np.array(cond, copy=True)
    for i in range(tree.n):
        if tree.parent[i] >= 0:
            out[..., i] = out[..., tree.parent[i]] * out[..., i]
    return out


def top_prediction(cond, tree, thresh, return_margins=False):
    """cond [n] of one row -> (node, abs[node]): walk down from the root group while the product stays above thresh.
    With return_margins a third value: {"thresh": the least |p cond[j] - thresh| over the steps taken, "group_gap": the
    least gap between the two largest cond of a visited group (inf for a group of one)}"""
    cond = np.asarray(cond)
    assert cond.shape == (tree.n,), cond.shape
    margins = {"thresh": np.inf, "group_gap": np.inf}
    p, g = cond.dtype.type(1.0), 0
    while True:
        off, size = int(tree.group_offset[g]), int(tree.group_size[g])
        v = cond[off:off + size]
        j = off + int(np.argmax(v))                              # first maximum
        if size > 1:
            two = np.sort(v)[-2:]
            margins["group_gap"] = min(margins["group_gap"], float(two[1] - two[0]))
        margins["thresh"] = min(margins["thresh"], abs(float(p * cond[j]) - thresh))
        if p * cond[j] > thresh:
            p = p * cond[j]
            if tree.child[j] < 0:
                node = j
                break
            g = int(tree.child[j])
            continue
        if g == 0:                                               # the root group always answers
            node, p = j, p * cond[j]
        else:
            node = int(tree.parent[off])                         # the node whose children were not convincing
        break
    return (node, p, margins) if return_margins else (node, p)


def path_to_root(tree, k):
    """k, parent[k], ... up to a root"""
    out = []
    while k >= 0:
        out.append(int(k))
        k = int(tree.parent[k])
    return out


def yolov2_loss_boxes_tree(net, truth, ntruth, anchors, image_size, tree, coord_scale=1.0, object_scale=5.0,
                           noobject_scale=1.0, class_scale=1.0, thresh=0.6, area_weight=False, prior_scale=0.0,
                           dtype=np.float64, return_margins=False):
    """utils/region_loss.py yolov2_loss_boxes with the class term of an owned slot replaced: for each node a of the path
    k, parent[k], ... of the truth's class k (0 <= k < C), with g = group[a], parts[3] += class_scale (lse_g - logit[a])
    and dnet = class_scale (softmax_g - onehot(a)) over the members of g; every other class entry gets gradient 0.  That
    is -class_scale log(abs[k])."""
    from .region_loss import yolov2_loss_boxes
    net = np.asarray(net, dtype)
    n, s, _, b, d = net.shape
    c = d - 5
    assert tree.n == c, (tree.n, c)
    # everything but the class term: the flat loss with class_scale = 0 (its class part and class gradient are then 0)
    loss, dnet, margins = yolov2_loss_boxes(net, truth, ntruth, anchors, image_size, coord_scale, object_scale,
                                            noobject_scale, 0.0, thresh, area_weight, prior_scale, dtype, True)
    dnet[..., 5:] = 0.0                                          # (-0.0 of the zero scale)
    truth = np.asarray(truth, dtype)
    ntruth = np.asarray(ntruth).astype(np.int64)
    an = np.asarray(anchors, dtype)
    cls = dtype(0.0)
    for i in range(n):
        owned = set()
        for k in range(int(ntruth[i])):
            tr = truth[i, k]
            gx, gy = tr[0] / image_size * s, tr[1] / image_size * s
            gw, gh = tr[2] / image_size * s, tr[3] / image_size * s
            r, q = min(int(gy), s - 1), min(int(gx), s - 1)
            bs = int(np.argmax(shape_ious(gw, gh, an)))
            if (r, q, bs) in owned:
                continue
            owned.add((r, q, bs))
            node = int(tr[4])
            if not 0 <= node < c:
                continue
            lg = net[i, r, q, bs, 5:]
            for a in path_to_root(tree, node):
                g = int(tree.group[a])
                off, size = int(tree.group_offset[g]), int(tree.group_size[g])
                v = lg[off:off + size]
                m = v.max()
                lse = m + np.log(np.exp(v - m).sum())
                cls += class_scale * (lse - lg[a])
                sm = np.exp(v - lse)
                sm[a - off] -= 1.0
                dnet[i, r, q, bs, 5 + off:5 + off + size] = class_scale * sm / n
    parts = np.array([loss[0], loss[1], loss[2], cls / n], dtype)
    loss = np.concatenate([parts, [parts.sum()]]).astype(dtype)
    return (loss, dnet, margins) if return_margins else (loss, dnet)


def region_stats_boxes_tree(net, truth, ntruth, anchors, image_size, tree, dtype=np.float64, return_margins=False):
    """utils/region_loss.py region_stats_boxes with the class statistic = abs[k] of the truth's node (Darknet's avg_cat)"""
    from .region_loss import region_stats_boxes
    net = np.asarray(net, dtype)
    n, s, _, b, d = net.shape
    c = d - 5
    assert tree.n == c, (tree.n, c)
    stats, margins = region_stats_boxes(net, truth, ntruth, anchors, image_size, dtype, True)
    truth = np.asarray(truth, dtype)
    ntruth = np.asarray(ntruth).astype(np.int64)
    an = np.asarray(anchors, dtype)
    clss = []
    for i in range(n):
        for k in range(int(ntruth[i])):
            tr = truth[i, k]
            gx, gy = tr[0] / image_size * s, tr[1] / image_size * s
            gw, gh = tr[2] / image_size * s, tr[3] / image_size * s
            r, q = min(int(gy), s - 1), min(int(gx), s - 1)
            bs = int(np.argmax(shape_ious(gw, gh, an)))
            node = int(tr[4])
            if 0 <= node < c:
                clss.append(absolute(conditional(net[i, r, q, bs, 5:], tree, dtype), tree)[node])
    stats = stats.copy()
    stats[1] = float(np.mean(np.asarray(clss, dtype))) if clss else 0.0
    return (stats, margins) if return_margins else stats


def word_tree_head(net, tree, tree_thresh, dtype=np.float64, return_margins=False):
    """net [rows][5 + C] -> (out, top int64 [rows], prob [rows]): elements 0..4 copied, the class logits replaced by 0 at
    top = top_prediction(conditional(logits), tree_thresh) and -inf everywhere else; prob = abs[top].  Every detect
    entry reads such a row as score sig(to) at top and 0 elsewhere.  With return_margins a fourth value: the least of
    each margin of top_prediction over the rows"""
    net = np.asarray(net)
    rows, d = net.shape
    assert d == 5 + tree.n, (d, tree.n)
    out = np.full(net.shape, -np.inf, net.dtype)
    out[:, :5] = net[:, :5]
    top = np.zeros(rows, np.int64)
    prob = np.zeros(rows, dtype)
    margins = {"thresh": np.inf, "group_gap": np.inf}
    cond = conditional(net[:, 5:], tree, dtype)
    for r in range(rows):
        node, p, m = top_prediction(cond[r], tree, tree_thresh, True)
        top[r], prob[r] = node, p
        out[r, 5 + node] = 0.0
        for k in margins:
            margins[k] = min(margins[k], m[k])
    return (out, top, prob, margins) if return_margins else (out, top, prob)
