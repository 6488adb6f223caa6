"""The wide head on the host (no GPU): utils/darknet_cfg.py under wide_head=True -- `map=`, `tree=`, a last convolution
wider than a stack's row -- on tests/golden/cfg/chain-wide.cfg and on YOLO9000's cfg as remembered, and everything the
keyword must leave alone."""
import pytest

import _wide_head_cases as K
from tensorflow_yolo2_amd.utils import darknet_cfg as C, word_tree as W
from tensorflow_yolo2_amd.utils.darknet_weights import layer_floats


def test_the_700_node_tree_has_the_shapes_the_kernels_meet():
    tree = W.parse(K.wide700_text(), "<wide700>")
    assert tree.n == 700 and len(tree.group_offset) == 50 and max(tree.group_size) == 70 and tree.max_depth == 4


def test_default_keyword_keeps_todays_refusals(tmp_path):
    cfg = K.write_wide_model_files(tmp_path)
    with pytest.raises(ValueError) as e:
        C.load(cfg)
    assert "map=x.map" in str(e.value) and "wide head" in str(e.value).replace("-", " ")
    bare = K.write_wide_model_files(tmp_path, with_map=False)
    with pytest.raises(ValueError) as e:
        C.load(bare)
    assert "at most 2048" in str(e.value) and "width 2115" in str(e.value)
    with pytest.raises(ValueError, match="at most 2048"):
        C.compile_graph(C.load(bare, wide_head=True))                    # the record parses; the default compile refuses


def test_wide_head_keyword_reads_map_and_cuts_the_head(tmp_path):
    record = C.load(K.write_wide_model_files(tmp_path), wide_head=True)
    assert record.map == "x.map" and record.tree == "wide700.tree" and record.classes == 700 and record.num == 3
    graph = C.compile_graph(record, wide_head=True)
    assert graph.wide is True and graph.shape == "chain" and graph.pool == "s1" and graph.head_layers == 3
    assert graph.specs[-1] == ((3, 64, 128, 0), (3, 128, 128, 0))        # the head stack ends at the 128-wide layer
    assert len(graph.file_layers) == 9 and graph.file_layers[-1] == (1, 128, 2115, False)
    assert record.file_layers == graph.file_layers
    assert record.floats == sum(layer_floats(l) for l in graph.file_layers)
    assert record.floats == sum(n * c * k * k + (4 * n if bn else n) for (k, c, n, bn) in graph.file_layers)
    # fp32 storage: the stacks' limit is 1024, the last layer is wide there too
    assert C.compile_graph(record, 1024, wide_head=True).wide is True


def test_a_narrow_cfg_compiles_the_same_with_and_without_the_keyword():
    a, b = C.load(K.CHAIN_TREE_CFG), C.load(K.CHAIN_TREE_CFG, wide_head=True)
    assert a == b and a.map is None
    ga, gb = C.compile_graph(a), C.compile_graph(b, wide_head=True)
    assert ga == gb and ga.wide is False and ga.head_layers == 3 and len(ga.specs[-1]) == 3
    assert ga._fields[:8] == ("shape", "specs", "file_layers", "centre_tap", "narrow", "head_layers", "pool", "route")


def _line_of(text, item):
    return 1 + text.splitlines().index(item)


def test_tree_is_a_synonym_of_softmax_tree():
    with open(K.CHAIN_TREE_CFG) as f:
        text = f.read()
    same = text.replace("softmax_tree=../tree/small.tree", "tree=../tree/small.tree")
    assert same != text
    assert C.parse(same, "x.cfg").tree == "../tree/small.tree" == C.parse(text, "x.cfg").tree
    both = text.replace("softmax_tree=../tree/small.tree", "softmax_tree=../tree/small.tree\ntree=../tree/small.tree")
    assert C.parse(both, "x.cfg").tree == "../tree/small.tree"
    bad = text.replace("softmax_tree=../tree/small.tree", "softmax_tree=../tree/small.tree\ntree=other.tree")
    for wide in (False, True):
        with pytest.raises(ValueError) as e:
            C.parse(bad, "x.cfg", wide_head=wide)
        assert "x.cfg:%d:" % _line_of(bad, "tree=other.tree") in str(e.value) and "other.tree" in str(e.value)
        assert "../tree/small.tree" in str(e.value)


def test_batch_norm_layers_keep_the_row_limit_under_the_keyword(tmp_path):
    with open(K.write_wide_model_files(tmp_path)) as f:
        text = f.read()
    assert text.count("filters=128\n") == 2
    head, _, tail = text.rpartition("filters=128\n")
    bad = head + "filters=4096\n" + tail                                  # the conv-BN-leaky layer in front of the wide one
    with pytest.raises(ValueError) as e:
        C.parse(bad, "x.cfg", wide_head=True)
    assert "width 4096 (filters): at most 2048" in str(e.value) and "layer 13 [convolutional]" in str(e.value)
    # the wide layer's INPUT keeps the inner rules: 100 is no multiple of 32
    bad = head + "filters=100\n" + tail
    with pytest.raises(ValueError, match="multiple of 32"):
        C.parse(bad, "x.cfg", wide_head=True)


def test_yolo9000_cfg_as_remembered_compiles():
    text = K.yolo9000_cfg_text()
    with pytest.raises(ValueError, match="map"):
        C.parse(text, "yolo9000.cfg")
    record = C.parse(text, "yolo9000.cfg", wide_head=True)
    assert (record.size, record.classes, record.num) == (544, 9418, 3)
    assert record.tree == "data/9k.tree" and record.map == "data/coco9k.map" and record.tree_thresh == 0.5
    graph = C.compile_graph(record, wide_head=True)
    assert graph.wide and graph.shape == "chain" and graph.pool == "s2"
    assert len(graph.file_layers) == 19 and graph.file_layers[-1] == (1, 1024, 28269, False)
    assert [len(s) for s in graph.specs] == [13, 5] and graph.specs[-1][-1] == (3, 512, 1024, 0)
    assert graph.centre_tap == (3,)                   # Darknet-19's fourth layer: 1x1 in the file, behind two pools
    widths, cin, floats = [], 3, 0
    for (k, n, _pool) in K.YOLO9000_CONVS:
        floats += n * cin * k * k + 4 * n
        cin = n
    floats += 28269 * 1024 + 28269
    assert record.floats == floats == sum(layer_floats(l) for l in graph.file_layers)
    assert 28269 == 3 * (5 + 9418)
