"""The word tree on the host (utils/word_tree.py, no GPU): the tree file and its refusals, the hierarchical loss against the
flat one, against -log abs[k] and against finite differences, top_prediction's walk, and the cfg keys that name a tree."""
import os

import numpy as np
import pytest

import _word_tree_cases as K
from tensorflow_yolo2_amd.utils import darknet_cfg as C, region_loss as RL, word_tree as W


# ---------------------------------------------------------------- the tree file
def test_small_tree_tables_by_hand():
    t = K.small_tree()
    assert t.n == 20 and t.max_depth == 2 and W.groups(t) == 7
    assert t.labels[:5] == ("animal", "vehicle", "person", "furniture", "dog") and t.labels[-1] == "van"
    assert t.parent.tolist() == [-1, -1, -1, -1, 0, 0, 0, 0, 1, 1, 1, 3, 4, 4, 4, 5, 5, 8, 8, 8]
    assert t.group.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 4, 4, 4, 5, 5, 6, 6, 6]
    assert t.group_offset.tolist() == [0, 4, 8, 11, 12, 15, 17]
    assert t.group_size.tolist() == [4, 4, 3, 1, 3, 2, 3]                      # a root group of four, a group of one
    assert t.child.tolist() == [1, 2, -1, 3, 4, 5, -1, -1, 6, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1]
    assert t.depth.tolist() == [0] * 4 + [1] * 8 + [2] * 8
    assert t.child[2] == -1 and t.depth[2] == 0                                # a leaf at depth 0
    packed = W.pack(t)
    assert packed.dtype == np.int32 and packed.shape == (3 * 20 + 2 * 7,)
    assert packed[:20].tolist() == t.parent.tolist() and packed[20:40].tolist() == t.group.tolist()
    assert packed[40:60].tolist() == t.child.tolist()
    assert packed[60:67].tolist() == t.group_offset.tolist() and packed[67:].tolist() == t.group_size.tolist()
    assert W.path_to_root(t, 18) == [18, 8, 1] and W.path_to_root(t, 2) == [2]


def test_wide_tree_has_the_groups_the_kernels_are_tested_on():
    t = K.wide_tree()
    assert t.n == 70 and t.max_depth == 2 and t.group_size.tolist() == [3, 65, 1, 1]
    assert t.parent[68] == 1 and t.parent[69] == 3 and t.child[3] == 3 and t.child[1] == 2


@pytest.mark.parametrize("text,line,word", [
    ("", 1, "no node"),
    ("\n\n  \n", 3, "no node"),
    ("a 0\n", 1, "not below"),
    ("a -1\n\nb 2\n", 3, "not below"),
    ("a -1\nb -2\n", 2, "neither a node index nor -1"),
    ("a -1\nb x\n", 2, "no integer"),
    ("a -1\nb\n", 2, "label parent"),
    ("a -1\nb 0 c\n", 2, "label parent"),
    ("a -1\nb 0\n\nc -1\n", 4, "roots come first"),
    ("a -1\nb -1\nc 0\nd 1\ne 0\n", 5, "not consecutive"),
])
def test_tree_refusals_name_the_line(text, line, word):
    with pytest.raises(ValueError) as e:
        W.parse(text, "some.tree")
    assert str(e.value).startswith("some.tree:%d: " % line) and word in str(e.value), str(e.value)


def test_blank_lines_do_not_number_nodes():
    t = W.parse("\na -1\n\n\nb 0\n")
    assert t.n == 2 and t.parent.tolist() == [-1, 0] and t.group_size.tolist() == [1, 1]


# ---------------------------------------------------------------- probabilities
def test_conditional_and_absolute():
    t = K.small_tree()
    rng = np.random.default_rng(0)
    lg = rng.standard_normal((3, 20))
    cond = W.conditional(lg, t)
    for off, size in zip(t.group_offset, t.group_size):
        np.testing.assert_allclose(cond[:, off:off + size].sum(axis=1), 1.0, rtol=1e-12)
    assert (cond[:, 11] == 1.0).all()                                          # the group of one
    ab = W.absolute(cond, t)
    np.testing.assert_allclose(ab[:, 18], cond[:, 1] * cond[:, 8] * cond[:, 18], rtol=1e-12)
    np.testing.assert_allclose(ab[:, :4], cond[:, :4])
    leaves = t.child < 0
    np.testing.assert_allclose(ab[:, leaves].sum(axis=1), 1.0, rtol=1e-12)     # the leaves partition the probability


def _cond(t, winners, strength):
    """conditionals whose maximum of each listed group is the listed node, with cond = strength (others share the rest)"""
    cond = np.zeros(t.n)
    for g, (off, size) in enumerate(zip(t.group_offset, t.group_size)):
        cond[off:off + size] = 1.0 / size
    for node, s in zip(winners, strength):
        g = t.group[node]
        off, size = t.group_offset[g], t.group_size[g]
        if size > 1:
            cond[off:off + size] = (1.0 - s) / (size - 1)
            cond[node] = s
    return cond


def test_top_prediction_walks():
    t = K.small_tree()
    # thresh 0: greedy to a leaf
    cond = _cond(t, (1, 8, 18), (0.6, 0.5, 0.7))
    node, p, m = W.top_prediction(cond, t, 0.0, return_margins=True)
    assert node == 18 and p == pytest.approx(0.6 * 0.5 * 0.7)
    assert m["thresh"] == pytest.approx(0.21) and m["group_gap"] == pytest.approx(0.25)   # 0.5 against 0.25 in the cars
    # a stop below the root returns the parent: 0.6 * 0.5 = 0.3 does not pass 0.4
    node, p = W.top_prediction(cond, t, 0.4)
    assert node == 1 and p == pytest.approx(0.6)
    # one level further: 0.3 passes 0.25, 0.21 does not
    node, p = W.top_prediction(cond, t, 0.25)
    assert node == 8 and p == pytest.approx(0.3)
    # a thresh no product exceeds: the root group's maximum answers, with its own probability
    node, p, m = W.top_prediction(cond, t, 0.95, return_margins=True)
    assert node == 1 and p == pytest.approx(0.6) and m["thresh"] == pytest.approx(0.35)
    # a leaf at depth 0
    node, p = W.top_prediction(_cond(t, (2,), (0.7,)), t, 0.5)
    assert node == 2 and p == pytest.approx(0.7)
    # a group of one: furniture -> chair with cond 1, margins see no gap there
    node, p, m = W.top_prediction(_cond(t, (3,), (0.7,)), t, 0.5, return_margins=True)
    assert node == 11 and p == pytest.approx(0.7) and m["group_gap"] == pytest.approx(0.6)
    one = W.parse("only -1\n")
    node, p, m = W.top_prediction(np.ones(1), one, 0.5, return_margins=True)
    assert node == 0 and p == 1.0 and m["group_gap"] == np.inf
    # the first maximum of a tie
    tie = _cond(t, (), ())
    assert W.top_prediction(tie, t, 0.9)[0] == 0 and W.top_prediction(tie, t, 0.0)[0] == 12


def test_word_tree_head_rows():
    for name in ("small", "wide"):
        net, tree = K.head_input(name)
        for thresh in (0.0, 0.5, 0.9):
            out, top, prob, m = W.word_tree_head(net, tree, thresh, return_margins=True)
            assert min(m.values()) >= K.MARGIN, (name, thresh, m)
            assert np.array_equal(out[:, :5].view(np.uint32), net[:, :5].view(np.uint32))
            assert ((out[:, 5:] == 0).sum(axis=1) == 1).all() and (np.isneginf(out[:, 5:]).sum(axis=1) == tree.n - 1).all()
            assert np.array_equal(np.argmax(out[:, 5:], axis=1), top)
            ab = W.absolute(W.conditional(net[:, 5:], tree), tree)
            np.testing.assert_allclose(prob, ab[np.arange(len(top)), top], rtol=1e-12)
            if thresh == 0.0:
                assert (tree.child[top] < 0).all()
        # the thresholds stop walks at different levels
        tops = [W.word_tree_head(net, tree, th)[1] for th in (0.0, 0.5, 0.9)]
        assert tree.depth[tops[0]].mean() > tree.depth[tops[1]].mean() > tree.depth[tops[2]].mean()


# ---------------------------------------------------------------- the loss
def test_one_group_is_the_flat_loss():
    net, truth, ntruth, anchors, size, tree = K.parity_input("n3_S5_small")
    flat = W.flat(tree.n)
    assert W.groups(flat) == 1 and flat.max_depth == 0
    for kw in ({}, dict(area_weight=True, prior_scale=0.01, **K.NONDEFAULT)):
        a_loss, a_d = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, flat, **kw)
        b_loss, b_d = RL.yolov2_loss_boxes(net, truth, ntruth, anchors, size, **kw)
        np.testing.assert_allclose(a_loss, b_loss, rtol=1e-12)
        np.testing.assert_allclose(a_d, b_d, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("key", sorted(K.SHAPES))
def test_class_part_is_minus_log_abs_of_the_owners(key):
    net, truth, ntruth, anchors, size, tree = K.parity_input(key)
    n, S = net.shape[0], net.shape[1]
    scale = 1.5
    loss, dnet = K.checked_loss(net, truth, ntruth, anchors, size, tree, class_scale=scale)
    own = K.owners(truth, ntruth, anchors, size, S)
    assert len(own) < ntruth.sum()                                             # some truths lost their slot
    total = 0.0
    on_path = np.zeros(dnet.shape, bool)
    for (i, r, q, b, k, _index) in own:
        ab = W.absolute(W.conditional(net[i, r, q, b, 5:], tree), tree)
        total += -scale * np.log(ab[k])
        for a in W.path_to_root(tree, k):
            g = tree.group[a]
            on_path[i, r, q, b, 5 + tree.group_offset[g]:5 + tree.group_offset[g] + tree.group_size[g]] = True
    np.testing.assert_allclose(loss[3], total / n, rtol=1e-12)
    # everything but the class part is the flat loss's, and no class entry off a path has a gradient
    f_loss, f_d = RL.yolov2_loss_boxes(net, truth, ntruth, anchors, size, class_scale=scale)
    np.testing.assert_allclose(loss[:3], f_loss[:3], rtol=1e-12)
    assert np.array_equal(dnet[..., :5], f_d[..., :5])
    cls = np.zeros(dnet.shape, bool)
    cls[..., 5:] = True
    assert not dnet[cls & ~on_path].any() and dnet[on_path].any()


def test_gradient_is_the_finite_difference_of_the_loss():
    net, truth, ntruth, anchors, size, tree = K.parity_input("n3_S5_small")
    net = net.astype(np.float64)
    kw = dict(area_weight=True, **K.NONDEFAULT)
    _, dnet = W.yolov2_loss_boxes_tree(net, truth, ntruth, anchors, size, tree, **kw)
    own = K.owners(truth, ntruth, anchors, size, net.shape[1])
    deep = next(o for o in own if tree.depth[o[4]] == 2)
    i, r, q, b, k = deep[:5]
    path = W.path_to_root(tree, k)
    sibling = next(j for j in range(tree.n) if tree.group[j] == tree.group[path[1]] and j != path[1])
    off_path = next(j for j in range(tree.n) if tree.group[j] not in [tree.group[a] for a in path])
    free = next((ii, rr, qq, bb) for ii in range(net.shape[0]) for rr in range(net.shape[1]) for qq in range(net.shape[2])
                for bb in range(net.shape[3]) if (ii, rr, qq, bb) not in {o[:4] for o in own})
    eps = 1e-6
    for where, zero in ((deep[:4] + (5 + k,), False), (deep[:4] + (5 + path[1],), False), (deep[:4] + (5 + path[2],), False),
                        (deep[:4] + (5 + sibling,), False), (deep[:4] + (5 + off_path,), True), (free + (5 + k,), True)):
        hi, lo = net.copy(), net.copy()
        hi[where] += eps
        lo[where] -= eps
        fd = (W.yolov2_loss_boxes_tree(hi, truth, ntruth, anchors, size, tree, **kw)[0][4] -
              W.yolov2_loss_boxes_tree(lo, truth, ntruth, anchors, size, tree, **kw)[0][4]) / (2 * eps)
        if zero:
            assert dnet[where] == 0.0 and abs(fd) < 1e-9, (where, fd)
        else:
            assert dnet[where] != 0.0
            np.testing.assert_allclose(fd, dnet[where], rtol=1e-6)


def test_stats_class_is_the_mean_abs_of_every_truth():
    net, truth, ntruth, anchors, size, tree = K.parity_input("n2_S8_B3_wide")
    stats = K.checked_stats(net, truth, ntruth, anchors, size, tree)
    flat = RL.region_stats_boxes(net, truth, ntruth, anchors, size)
    assert np.array_equal(np.delete(stats, 1), np.delete(flat, 1)) and stats[1] != flat[1] and 0 < stats[1] < 1
    one = W.region_stats_boxes_tree(net, truth, ntruth, anchors, size, W.flat(tree.n))
    np.testing.assert_allclose(one, flat, rtol=1e-12)


# ---------------------------------------------------------------- the cfg
def test_cfg_accepts_the_tree_keys():
    rec = C.load(K.CHAIN_TREE_CFG)
    assert rec.tree == "../tree/small.tree" and rec.tree_thresh == 0.4 and rec.classes == 20 and rec.num == 3
    plain = C.load(os.path.join(os.path.dirname(K.CHAIN_TREE_CFG), "narrow-tiny.cfg"))
    assert plain.tree is None and plain.tree_thresh == 0.5                     # Darknet's -hier default
    assert C.REFUSED_REGION_KEYS == ("map",)
    text = open(K.CHAIN_TREE_CFG).read()
    line_of = lambda t, s: 1 + [l.replace(" ", "") for l in t.splitlines()].index(s)
    bad = text + "map=data/coco9k.map\n"
    with pytest.raises(ValueError) as e:
        C.parse(bad, "x.cfg")
    assert "x.cfg:%d:" % line_of(bad, "map=data/coco9k.map") in str(e.value) and "wide head" in str(e.value).replace("-", " ")
    for value in ("1", "-0.1", "1.5"):
        bad = text.replace("tree_thresh=0.4", "tree_thresh=%s" % value)
        with pytest.raises(ValueError) as e:
            C.parse(bad, "x.cfg")
        assert "x.cfg:%d:" % line_of(bad, "tree_thresh=%s" % value) in str(e.value) and "tree_thresh" in str(e.value)


def test_from_cfg_finds_the_tree_and_checks_its_size(tmp_path, monkeypatch):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    rec = C.load(K.CHAIN_TREE_CFG)
    tree = yolov2.load_cfg_tree(rec)                                           # relative to the cfg's directory
    assert tree.n == 20 and tree.labels[19] == "van"
    assert yolov2.load_cfg_tree(C.load(os.path.join(os.path.dirname(K.CHAIN_TREE_CFG), "narrow-tiny.cfg"))) is None
    # the working directory comes first
    text = open(K.CHAIN_TREE_CFG).read()
    cfg_dir, cwd = tmp_path / "cfg", tmp_path / "cwd"
    for d in (cfg_dir, cwd, tmp_path / "tree"):
        d.mkdir()
    (cfg_dir / "t.cfg").write_text(text.replace("../tree/small.tree", "names.tree"))
    (cfg_dir / "names.tree").write_text(open(K.SMALL_TREE).read())
    (cwd / "names.tree").write_text(open(K.SMALL_TREE).read().replace("van", "lorry"))
    monkeypatch.chdir(cwd)
    assert yolov2.load_cfg_tree(C.load(str(cfg_dir / "t.cfg"))).labels[19] == "lorry"
    # a tree of another size is refused at from_cfg, before anything is built
    (cwd / "names.tree").write_text("a -1\nb -1\nc 0\n")
    for make in (yolov2.YOLOv2Detector.from_cfg, yolov2.YOLOv2DarknetTrainer.from_cfg):
        with pytest.raises(ValueError) as e:
            make(str(cfg_dir / "t.cfg"), 2, dtype="f32")
        assert "3 nodes" in str(e.value) and "classes=20" in str(e.value)
    # a missing file names both places
    (cfg_dir / "m.cfg").write_text(text.replace("../tree/small.tree", "missing.tree"))
    with pytest.raises(ValueError) as e:
        yolov2.YOLOv2Detector.from_cfg(str(cfg_dir / "m.cfg"), 2, dtype="f32")
    assert "missing.tree" in str(e.value) and os.path.join(str(cfg_dir), "missing.tree") in str(e.value)


def test_command_line_flags_beat_the_file(tmp_path, capsys):
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2 as D, pascal_eval_yolov2 as EV, pascal_train_yolov2 as T
    other, three = tmp_path / "other.tree", tmp_path / "three.tree"
    other.write_text(open(K.SMALL_TREE).read().replace("van", "lorry"))
    three.write_text("a -1\nb -1\nc 0\n")
    base = ["--devkit", "x", "--cfg", K.CHAIN_TREE_CFG]
    a = T.parse_args(base)
    assert a.tree_record.n == 20 and a.tree_record.labels[19] == "van" and a.hier_thresh == 0.4
    a = T.parse_args(base + ["--tree", str(other), "--hier-thresh", "0.7"])
    assert a.tree_record.labels[19] == "lorry" and a.hier_thresh == 0.7
    a = T.parse_args(["--devkit", "x"])
    assert a.tree_record is None and a.hier_thresh == 0.5
    assert T.parse_args(["--devkit", "x", "--box-labels", "--tree", K.SMALL_TREE]).tree_record.n == 20
    for bad in (["--devkit", "x", "--tree", K.SMALL_TREE],                   # a tree needs the box list
                base + ["--tree", str(three)], base + ["--hier-thresh", "1.0"], base + ["--tree", str(tmp_path / "no.tree")]):
        with pytest.raises(SystemExit):
            T.parse_args(bad)
    for mod in (EV, D):
        rest = ["--darknet-weights", "w.weights"] + ([] if mod is EV else ["--images", "a.jpg"])
        a = mod.parse_args((["--devkit", "x"] if mod is EV else []) + ["--cfg", K.CHAIN_TREE_CFG] + rest)
        assert a.tree_record.n == 20 and a.hier_thresh == 0.4
        a = mod.parse_args((["--devkit", "x"] if mod is EV else []) + ["--cfg", K.CHAIN_TREE_CFG, "--tree", str(other),
                                                                      "--hier-thresh", "0.2"] + rest)
        assert a.tree_record.labels[19] == "lorry" and a.hier_thresh == 0.2
    capsys.readouterr()
