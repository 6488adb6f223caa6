"""Darknet's cfg files on the host (utils/darknet_cfg.py): the grammar on small strings, every refusal with its line and
layer, the four full-width cfgs of tests/golden/cfg with their float counts, the solver a [net] section becomes, and
region_stats_boxes (utils/region_loss.py) against a loop-free restatement on a hand-made case.

The cfgs under tests/golden/cfg were written by hand for this repository from the layer tables of
yolo2_nets/yolov2.py (yolov2_darknet_specs, TINY_WIDTHS); no Darknet file was at hand."""
import os

import numpy as np
import pytest

from tensorflow_yolo2_amd.utils import darknet_cfg as C
from tensorflow_yolo2_amd.utils import darknet_weights as DW
from tensorflow_yolo2_amd.utils import region_loss as RL
from tensorflow_yolo2_amd.utils.solver import Solver

NET = "[net]\nwidth=64\nheight=64\nchannels=3\nbatch=2\n"
CONV = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=3\nstride=1\npad=1\nactivation=leaky\n"
POOL = "[maxpool]\nsize=2\nstride=2\n"
LAST = "[convolutional]\nfilters=%d\nsize=1\nstride=1\npad=1\nactivation=linear\n"
REGION = "[region]\nanchors=1,2,3,4\nclasses=2\nnum=2\ncoords=4\nsoftmax=1\nbias_match=1\nrescore=1\n"


def chain(widths=(32, 32, 32, 32, 32, 64, 64), net=NET, region=REGION, out=14, tail=""):
    """a small chain: pools behind the first five layers, the rest is the head"""
    body = ""
    for i, w in enumerate(widths):
        body += CONV % w + (POOL if i < 5 else "")
    return net + body + LAST % out + region + tail


def passthrough(route_line="layers=-9", join_line="layers=-1,-4", route_filters=32):
    """a small passthrough in yolov2-voc.cfg's layout: layer 16 is the fine map, 24 the last coarse convolution"""
    c = lambda n, k=3: (CONV % n).replace("size=3", "size=%d" % k)
    stem = (c(32) + POOL + c(32) + POOL + c(32) + c(32, 1) + c(32) + POOL + c(32) + c(32, 1) + c(32) + POOL +
            c(64) + c(32, 1) + c(64) + c(32, 1) + c(64) + POOL)
    deep = c(128) + c(64, 1) + c(128) + c(64, 1) + c(128) + c(128) + c(128)
    return (NET + stem + deep + "[route]\n%s\n" % route_line + c(route_filters, 1) + "[reorg]\nstride=2\n" +
            "[route]\n%s\n" % join_line + c(128) + LAST % 14 + REGION)


def refused(text, *words):
    with pytest.raises(ValueError) as e:
        C.parse(text, "some.cfg")
    msg = str(e.value)
    assert msg.startswith("some.cfg:"), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


def line_of(text, needle, nth=0):
    return [i for i, l in enumerate(text.splitlines(), 1) if l.strip().replace(" ", "") == needle][nth]


# ---------------------------------------------------------------- grammar
def test_grammar_comments_spaces_network_and_duplicates():
    text = chain()
    plain = C.parse(text)
    spaced = text.replace("[net]", "# a comment\n; another\n\n  [ network ]  ").replace("width=64", "  width =  64  ")
    spaced = spaced.replace("filters=64", "filters = 64").replace("batch=2", "batch=7\n# the later key wins\nbatch=2")
    rec = C.parse(spaced)
    unlined = lambda r: [l._replace(line=0) for l in r.layers]           # comments and blank lines move the line numbers
    assert unlined(rec) == unlined(plain) and rec.file_layers == plain.file_layers and rec.batch == 2 and rec.size == 64
    assert [l.index for l in rec.layers] == list(range(len(rec.layers))) and rec.layers[-1].kind == "region"
    assert rec.layers[0].kind == "convolutional" and dict(rec.layers[0].options)["filters"] == 32
    with pytest.raises(AttributeError):
        rec.batch = 3                                        # the record is immutable
    assert rec.anchors == ((1.0, 2.0), (3.0, 4.0)) and rec.classes == 2 and rec.num == 2
    assert C.parse(text.replace("anchors=1,2,3,4", "anchors = 1.0, 2.0,  3.0,4.0")).anchors == rec.anchors
    assert dict(rec.scales) == dict(coord_scale=1.0, object_scale=1.0, noobject_scale=1.0, class_scale=1.0, thresh=0.5)
    assert rec.file_layers[0] == (3, 3, 32, True) and rec.file_layers[-1] == (1, 64, 14, False)
    assert rec.floats == sum(DW.layer_floats(l) for l in rec.file_layers)
    refused("[convolutional]\nfilters=3\n" + text, "first section", "[net]")


def test_grammar_route_indices_and_lists():
    rel = C.parse(passthrough())
    ab = C.parse(passthrough("layers=16", "layers=27, 24"))
    assert rel.layers == ab.layers
    assert dict(rel.layers[25].options)["layers"] == (16,) and dict(rel.layers[28].options)["layers"] == (27, 24)
    g = C.compile_graph(rel)
    assert g.shape == "passthrough" and g.route and [len(s) for s in g.specs] == [13, 7, 1, 2] and g.centre_tap == (3,)
    assert g.specs[3][0][:3] == (3, 4 * 32 + 128, 128) and g.specs[2] == ((1, 64, 32, 0),)
    # the first-release layout: a route without its convolution -- the fine map itself is reorganised
    bare = passthrough().replace("[route]\nlayers=-9\n" + (CONV % 32).replace("size=3", "size=1"), "[route]\nlayers=-9\n")
    bare = bare.replace("layers=-1,-4", "layers=-1,-3")
    gb = C.compile_graph(C.parse(bare))
    assert not gb.route and [len(s) for s in gb.specs] == [13, 7, 2] and gb.specs[2][0][1] == 4 * 64 + 128
    text = chain(net=NET + "policy=steps\nsteps=100,200, 300\nscales=.1,.5,2\nlearning_rate=0.01\n")
    s = C.parse(text).solver
    assert s.steps == (100, 200, 300) and s.scales == (0.1, 0.5, 2.0) and s.policy == "steps"
    refused(text.replace("scales=.1,.5,2", "scales=.1,.5"), "[net]", "scales")


# ---------------------------------------------------------------- refusals
def test_refusals_name_the_line_and_the_layer():
    text = chain()
    bad = text.replace(POOL, "[avgpool]\n", 1)
    refused(bad, ":%d:" % line_of(bad, "[avgpool]"), "layer 1 [avgpool]", "not understood")
    for name in ("softmax", "cost", "yolo", "shortcut", "upsample"):
        refused(text.replace(POOL, "[%s]\n" % name, 1), "layer 1 [%s]" % name)
    bad = text.replace("pad=1\n", "pad=1\ngroups=2\n", 1)
    refused(bad, ":%d:" % line_of(bad, "groups=2"), "layer 0 [convolutional]", "unknown key groups=2")
    bad = text.replace("stride=1", "stride=2", 2).replace("stride=2", "stride=1", 1)        # the second convolution
    refused(bad, ":%d:" % line_of(bad, "stride=2", 1), "layer 2 [convolutional]", "stride=2")
    refused(text.replace("filters=64", "filters=sixty"), "filters=sixty", "integer")
    refused(text.replace("activation=leaky", "activation=relu", 1), "layer 0 [convolutional]", "activation=relu")
    n_region = len(C.parse(text).layers) - 1
    where = "layer %d [region]" % n_region
    for old, new, word in (("rescore=1", "rescore=0", "rescore=0"), ("coords=4", "coords=5", "coords=5"),
                           ("softmax=1", "softmax=0", "softmax=0"), ("bias_match=1", "bias_match=0", "bias_match=0"),
                           ("anchors=1,2,3,4", "anchors=1,2,3", "anchors holds 3 numbers")):
        bad = text.replace(old, new)
        refused(bad, ":%d:" % line_of(bad, new.replace(" ", "")), where, word)
    for key in C.REFUSED_REGION_KEYS:
        bad = text + "%s=data/9k.tree\n" % key
        refused(bad, ":%d:" % line_of(bad, "%s=data/9k.tree" % key), where, key)
    bad = text.replace("height=64", "height=96")
    refused(bad, ":%d:" % line_of(bad, "height=96"), "[net]", "height=96", "width=64")
    bad = text.replace("channels=3", "channels=1")
    refused(bad, ":%d:" % line_of(bad, "channels=1"), "[net]", "channels=1")
    refused(text.replace("batch=2", "batch=2\nangle=7"), "[net]", "angle")
    refused(text.replace("width=64", "width=80").replace("height=64", "height=80"), "[net]", "width=80", "multiple of 32")
    bad = chain(tail=CONV % 32)
    refused(bad, ":%d:" % line_of(bad, "[region]"), where, "must be the last section")
    # a width the executor cannot run: by layer, width and rule
    bad = chain(widths=(32, 32, 48, 32, 32, 64, 64))
    refused(bad, ":%d:" % line_of(bad, "[convolutional]", 2), "layer 4 [convolutional]", "48", "multiple of 32")
    bad = chain(widths=(32, 32, 32, 32, 32, 64, 192))
    refused(bad, "layer 12 [convolutional]", "input width 192", "multiple of 128")
    refused(chain(widths=(24, 32, 32, 32, 32, 64, 64)), "layer 0 [convolutional]", "first layer", "filters=24")
    refused(chain(out=15), "filters=15", "num (5 + classes)")
    refused(passthrough("layers=-8"), "layer 25 [route]", "fine map", "layer 16")
    refused(passthrough(join_line="layers=-4,-1"), "layer 28 [route]")
    refused(chain(widths=(32, 32, 32, 32, 32, 64, 4096)), "layer 11 [convolutional]", "4096", "at most 2048")


def test_wide_outputs_are_refused_in_fp32_storage_only():
    rec = C.parse(chain(widths=(32, 32, 32, 32, 32, 128, 2048)))
    assert C.compile_graph(rec).specs[1][1] == (3, 128, 2048, 0)
    with pytest.raises(ValueError) as e:
        C.compile_graph(rec, 1024)
    assert "2048" in str(e.value) and "fp32" in str(e.value) and "layer 11" in str(e.value)


# ---------------------------------------------------------------- the four full-width cfgs
def golden(golden_dir, name):
    return C.load(os.path.join(golden_dir, "cfg", name))


def test_full_width_cfgs_and_their_float_counts(golden_dir):
    """yolov2-voc: 50,676,061 and tiny-yolo-voc: 15,867,885 are the counts DESIGN.md states (darknet_graph_floats).
    yolov2 (COCO): the one layer that changes is the 1x1 output convolution on 1024 inputs, 125 -> 425 filters: 300 more
    filters of 1024 weights and one bias each, 50,676,061 + 300 * 1025 = 50,983,561.
    yolov2-tiny (COCO): against tiny-yolo-voc the eighth convolution 3x3 1024 -> 1024 with batch norm (9 * 1024 * 1024 +
    4 * 1024 = 9,441,280) becomes 1024 -> 512 (9 * 1024 * 512 + 4 * 512 = 4,720,640) and the output convolution 1x1
    1024 -> 125 (128,125) becomes 512 -> 425 (512 * 425 + 425 = 218,025): 15,867,885 - 9,441,280 - 128,125 + 4,720,640 +
    218,025 = 11,237,145."""
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    voc, tiny = golden(golden_dir, "yolov2-voc.cfg"), golden(golden_dir, "tiny-yolo-voc.cfg")
    coco, tiny_coco = golden(golden_dir, "yolov2.cfg"), golden(golden_dir, "yolov2-tiny.cfg")
    assert voc.floats == 50676061 == net_utils.darknet_graph_floats("darknet", 20, 5)
    assert tiny.floats == 15867885 == net_utils.darknet_graph_floats("tiny", 20, 5)
    assert coco.floats == 50983561 == 50676061 + 300 * 1025
    assert tiny_coco.floats == 11237145 == 15867885 - 9441280 - 128125 + 4720640 + 218025
    assert list(voc.file_layers) == DW.yolov2_voc_layers() and list(tiny.file_layers) == DW.yolov2_tiny_voc_layers()
    assert coco.classes == 80 and coco.file_layers[-1] == (1, 1024, 425, False) and coco.size == 608
    assert tiny_coco.classes == 80 and tiny_coco.file_layers[-2:] == ((3, 1024, 512, True), (1, 512, 425, False))
    # the compiled stacks are the named topologies'
    g = C.compile_graph(voc)
    assert [list(s) for s in g.specs] == [list(s) for s in yolov2.yolov2_darknet_specs(20, 5)]
    assert (g.centre_tap, g.narrow, g.head_layers, g.pool, g.route) == ((3,), (), 2, "s2", True)
    g = C.compile_graph(tiny)
    assert [list(s) for s in g.specs] == [list(s) for s in yolov2.yolov2_tiny_specs(20, 5)]
    assert (g.centre_tap, g.narrow, g.head_layers, g.pool) == ((), yolov2.TINY_NARROW, 3, "s1")
    np.testing.assert_array_equal(np.asarray(voc.anchors, np.float32), np.asarray(yolov2.ANCHORS_VOC, np.float32))
    np.testing.assert_array_equal(np.asarray(tiny.anchors, np.float32), np.asarray(yolov2.ANCHORS_TINY_VOC, np.float32))
    for name, div, topo in (("narrow-darknet.cfg", yolov2.yolov2_darknet_specs, "darknet"),
                            ("narrow-tiny.cfg", yolov2.yolov2_tiny_specs, "tiny")):
        rec = golden(golden_dir, name)
        assert [list(s) for s in C.compile_graph(rec).specs] == [list(s) for s in div(3, 5, 8)]
        assert list(rec.file_layers) == net_utils._file_layers(topo, div(3, 5, 8))


def test_net_section_becomes_the_solver(golden_dir):
    voc = golden(golden_dir, "yolov2-voc.cfg")
    assert voc.solver == Solver() and voc.max_batches == 80200          # max_batches reaches the Solver under poly only
    assert (voc.size, voc.batch, voc.subdivisions, voc.random) == (416, 64, 8, 1)
    assert voc.augmentation == C.Augmentation(jitter=0.3, hue=0.1, saturation=1.5, exposure=1.5)
    assert dict(voc.scales) == dict(coord_scale=1.0, object_scale=5.0, noobject_scale=1.0, class_scale=1.0, thresh=0.6)
    poly = golden(golden_dir, "poly.cfg")
    assert poly.solver == Solver(policy="poly", burn_in=10, power=2, steps=(), scales=(), max_batches=500)
    assert poly.max_batches == 500


def test_read_names(tmp_path):
    p = tmp_path / "three.names"
    p.write_text("aeroplane\n\n  traffic light  \nzebra\n")
    assert C.read_names(str(p)) == ["aeroplane", "traffic light", "zebra"]


# ---------------------------------------------------------------- region statistics
def test_region_stats_on_a_hand_made_case():
    """S = 2, B = 2, C = 3, size 64, anchors (1, 1) and (2, 1).  Image 0 holds three truths, image 1 one; every logit of
    the net is 0 but for the rows below, so sig = 1/2 and the decoded box of a slot is its anchor at the cell's centre.

      truth A  image 0, centre (16, 16) px = cell (0, 0) at (.5, .5), 32 x 32 px = 1 x 1 cells: anchor 0 (shape IoU 1).
               The prediction there is 1 x 1 at (.5, .5): IoU 1.  class 0, logits (ln 2, 0, 0): softmax 2/4 = 1/2.
               to = ln 3: sig = 3/4.
      truth B  image 0, the same box again (a second truth in the slot: it counts too), class 2: softmax 1/4.
      truth C  image 0, centre (48, 48) px = cell (1, 1) at (1.5, 1.5), 64 x 32 px = 2 x 1 cells: anchor 1.  tw = ln(2/5)
               there: the prediction is 4/5 x 1 inside the 2 x 1 truth, IoU 2/5 -- not above 0.5.  class 7: outside [0, 3),
               no class term.  to = 0: sig 1/2.
      truth D  image 1, centre (16, 48) px = cell (r 1, q 0) at (.5, 1.5), 32 x 32 px: anchor 0, tx such that sig(tx) =
               3/4: the prediction is shifted by 1/4 cell, intersection 3/4, union 5/4: IoU 3/5.  class 1, logits 0:
               1/3.  to = -ln 3: sig 1/4.

      avg IoU (1 + 1 + 2/5 + 3/5) / 4 = 3/4; class (1/2 + 1/4 + 1/3) / 3 = 13/36; obj (3/4 + 3/4 + 1/2 + 1/4) / 4 =
      9/16; no obj: 16 slots, 14 at 1/2, one at 3/4 (A and B share it), one at 1/4 (C's slot is 1/2 too): (14 / 2 + 3/4
      + 1/4) / 16 = 1/2; recall 3 of 4 (A, B, D); count 4."""
    anchors = ((1.0, 1.0), (2.0, 1.0))
    net = np.zeros((2, 2, 2, 2, 8))
    net[0, 0, 0, 0, 4], net[0, 0, 0, 0, 5] = np.log(3.0), np.log(2.0)
    net[0, 1, 1, 1, 2] = np.log(0.4)
    net[1, 1, 0, 0, 0], net[1, 1, 0, 0, 4] = np.log(3.0), -np.log(3.0)
    truth = np.zeros((2, 4, 5))
    truth[0, 0] = (16, 16, 32, 32, 0)
    truth[0, 1] = (16, 16, 32, 32, 2)
    truth[0, 2] = (48, 48, 64, 32, 7)
    truth[0, 3] = (5, 5, 5, 5, 1)                              # behind ntruth: not read
    truth[1, 0] = (16, 48, 32, 32, 1)
    ntruth = np.array([3, 1])
    want = np.array([3 / 4, 13 / 36, 9 / 16, 1 / 2, 3 / 4, 4.0])
    stats, margins = RL.region_stats_boxes(net, truth, ntruth, anchors, 64, return_margins=True)
    np.testing.assert_allclose(stats, want, rtol=1e-12)
    assert margins["iou_half"] == pytest.approx(0.1)           # truths C and D, on either side of the recall threshold
    assert margins["cell_edge"] == 0.5 and margins["shape_gap"] == pytest.approx(0.5)
    # the loop-free restatement: the same numbers from array expressions over the four truths
    sig = lambda v: 1 / (1 + np.exp(-v))
    img, row, col, anc = np.array([0, 0, 0, 1]), np.array([0, 0, 1, 1]), np.array([0, 0, 1, 0]), np.array([0, 0, 1, 0])
    g = np.array([[.5, .5, 1, 1], [.5, .5, 1, 1], [1.5, 1.5, 2, 1], [.5, 1.5, 1, 1]])
    cls = np.array([0, 2, 7, 1])
    t = net[img, row, col, anc]
    a = np.asarray(anchors)[anc]
    px, py, pw, ph = sig(t[:, 0]) + col, sig(t[:, 1]) + row, a[:, 0] * np.exp(t[:, 2]), a[:, 1] * np.exp(t[:, 3])
    iw = np.minimum(px + pw / 2, g[:, 0] + g[:, 2] / 2) - np.maximum(px - pw / 2, g[:, 0] - g[:, 2] / 2)
    ih = np.minimum(py + ph / 2, g[:, 1] + g[:, 3] / 2) - np.maximum(py - ph / 2, g[:, 1] - g[:, 3] / 2)
    inter = np.clip(iw, 0, None) * np.clip(ih, 0, None)
    iou = inter / (pw * ph + g[:, 2] * g[:, 3] - inter)
    soft = np.exp(t[:, 5:]) / np.exp(t[:, 5:]).sum(axis=1, keepdims=True)
    ok = (cls >= 0) & (cls < 3)
    direct = np.array([iou.mean(), soft[ok, cls[ok]].mean(), sig(t[:, 4]).mean(), sig(net[..., 4]).mean(),
                       (iou > 0.5).mean(), 4.0])
    np.testing.assert_allclose(stats, direct, rtol=1e-12)
    # a mean over nothing is 0
    empty = RL.region_stats_boxes(net, truth, np.zeros(2, np.int64), anchors, 64)
    np.testing.assert_array_equal(empty, [0, 0, 0, 0.5, 0, 0])
    assert RL.region_stats_boxes(net, truth, ntruth, anchors, 64, dtype=np.float32).dtype == np.float32
