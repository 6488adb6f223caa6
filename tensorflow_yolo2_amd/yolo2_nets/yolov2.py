"""YOLOv2 detector composed from the pieces of this library -- NOT in the reference (SURVEY.md §8 rows a-x1,
a-x2; the north star's model): Darknet-19 up to the 26x26x512 activation, 2x2 max pool, the 13x13 backbone
layers and two 3x3 head convolutions, the stride-2 passthrough (reorg 26x26x512 -> 13x13x2048, concatenated
with the 13x13x1024 path), a 3x3 convolution 3072 -> 1024, the 1x1 output convolution to B*(5+C) channels,
anchor-box decode and per-image NMS.  Every layer is the reference's conv-BN-leaky type (darknet.py:39-46),
so the three stacks are `engine.Network` contexts; the glue ops are csrc/ext.hip.  With `tree=` (a utils.word_tree.WordTree)
the class logits are the nodes of a word tree: csrc/word_tree.hip holds its loss, its statistics and its detection head.
`YOLOv2Detector` is the inference graph, `YOLOv2Trainer` the train step: anchor-box loss (csrc/ext.hip
yolov2_loss_kernel, specification oracle/ext_ref.py), backward through the head, the passthrough concat, the
13x13 stack, the 2x2 pool and the stem, Adam (or, with `solver`, Darknet's SGD: utils/solver.py) on the three flat
parameter buffers, optional multi-scale.  `YOLOv2DarknetTrainer` is the train step of the "darknet" topology, the graph
of yolov2-voc.cfg: four stacks, Darknet's reorg and its gradient, a last layer without batch statistics -- and, with
topology="tiny", of the "tiny" topology, the graph of tiny-yolo-voc.cfg: two stacks, Darknet's stride-1 pool between them
(engine.max_pool_2x2_s1), no passthrough, two narrow layers that run zero-padded.
`YOLOv2Detector.from_cfg` / `YOLOv2DarknetTrainer.from_cfg` build the graph a Darknet cfg describes (utils/darknet_cfg.py):
its layer list compiled onto the same record (_cfg_topology) -- a chain under the name "tiny", a passthrough under the name
"darknet" -- with the file's widths, class count and anchors.
"""
import collections

import numpy as np
import torch

from .. import engine as E

# k-means anchors of YOLOv2 on VOC, in 13x13 cell units (width, height)
ANCHORS_VOC = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))


def yolov2_specs(num_class=20, num_anchors=5, width_div=1):
    core = [tuple(s) for s in E.CORE_SPEC]
    a = core[:13]
    a[12] = (a[12][0], a[12][1], a[12][2], 0)            # keep the 26x26x512 activation un-pooled
    b = core[13:18] + [(3, 1024, 1024, 0), (3, 1024, 1024, 0)]
    c = [(3, 4 * 512 + 1024, 1024, 0), (1, 1024, num_anchors * (5 + num_class), 0)]
    if width_div > 1:      # narrow variant for tests: every inner width divided, the output width kept
        div = lambda ch: max(32, ch // width_div // 32 * 32)
        a = [(k, ci if i == 0 else div(ci), div(co), p) for i, (k, ci, co, p) in enumerate(a)]
        b = [(k, div(ci), div(co), p) for (k, ci, co, p) in b]
        c = [(3, 4 * a[-1][2] + b[-1][2], div(1024), 0), (1, div(1024), c[1][2], 0)]
    return a, b, c


DARKNET_BN_EPS = 1e-6            # Darknet's batch norm: (x - mean) / sqrt(var + .000001f)
DARKNET_ROUTE_WIDTH = 64         # the 1x1 convolution on the route of yolov2-voc.cfg: 512 -> 64, reorganised to 256


def yolov2_darknet_specs(num_class=20, num_anchors=5, width_div=1):
    """the four stacks of yolov2-voc.cfg: the stem and the 13x13 stack of yolov2_specs, the one-layer route stack on the
    fine map (its width stays 64 under width_div, its input is the divided one) and the head behind Darknet's
    passthrough: 3x3 over 4 * 64 + C13 channels, then the 1x1 output layer (linear, no batch norm in Darknet)"""
    a, b, c = yolov2_specs(num_class, num_anchors, width_div)
    r = [(1, a[-1][2], DARKNET_ROUTE_WIDTH, 0)]
    c = [(3, 4 * DARKNET_ROUTE_WIDTH + b[-1][2], c[0][2], 0), c[1]]
    return a, b, r, c


# tiny-yolo-voc.cfg (yolov2-tiny-voc.cfg): the anchors in 13x13 cell units, written down from memory of the cfg -- no
# file was at hand to confirm them ("Tiny YOLOv2")
ANCHORS_TINY_VOC = ((1.08, 1.19), (3.42, 4.41), (6.63, 11.38), (9.42, 5.11), (16.62, 10.52))
TINY_WIDTHS = (16, 32, 64, 128, 256, 512, 1024, 1024)    # the filters of its eight conv-BN-leaky layers, in the file
TINY_NARROW = ((0, 16),)         # (stem layer, filters in the file): the stack runs it 32 wide, the rest exactly zero


def yolov2_tiny_specs(num_class=20, num_anchors=5, width_div=1):
    """the two stacks of tiny-yolo-voc.cfg: six 3x3 layers with 2x2 / stride-2 pools behind the first five (Darknet's
    stride-1 pool behind the sixth runs between the stacks: engine.max_pool_2x2_s1), then 3x3, 3x3 and the 1x1 output
    layer.  The file's first two layers are 3 -> 16 and 16 -> 32; the stack's first layer is 3 -> 32 and inner input
    widths are multiples of 32, so they run as 3 -> 32 and 32 -> 32 with filters 16 .. 31 of the first and input
    channels 16 .. 31 of the second exactly zero (TINY_NARROW) -- the same function.  width_div divides the other widths
    only, so a narrow test model still exercises the padding."""
    div = (lambda ch: max(32, ch // width_div // 32 * 32)) if width_div > 1 else (lambda ch: ch)
    w = [32, 32] + [div(ch) for ch in TINY_WIDTHS[2:]]
    a = [(3, 3 if l == 0 else w[l - 1], w[l], 1 if l < 5 else 0) for l in range(6)]
    b = [(3, w[5], w[6], 0), (3, w[6], w[7], 0), (1, w[7], num_anchors * (5 + num_class), 0)]
    return a, b


TOPOLOGIES = ("paper", "darknet", "tiny")
DARKNET_FILE_TOPOLOGIES = ("darknet", "tiny")            # the graphs a Darknet `.weights` file can hold
DARKNET_1X1_CORE_LAYER = 3       # Darknet-19's fourth convolution: 1x1 in the file, 3x3 with a centre tap in this graph


def _paper_concat(fine, coarse, out=None):
    return E.passthrough_concat(fine, coarse)            # torch allocates the result: this path keeps no buffers


# What one YOLOv2 graph is, as data: everything below reads this record and never asks for the name.  Per stack, in
# networks() order: `heights` the input height in units of S = size / 32, `slopes` the activation slopes (None: 0.1
# everywhere), `train_options` the engine.Network options of a training context.  bn_eps: the default batch-norm epsilon
# (None: the contexts' own 1e-3).  head_statistics: whether the head trains on batch statistics.  darknet_input: uint8
# batches go through engine.u8_to_darknet_input into a buffer kept per size, and so does the concat; otherwise the first
# layer converts and torch allocates.  concat / concat_backward: the passthrough pair; cf_stack: the stack whose output
# width that pair reads as `cf` -- all three None on a graph without a passthrough, whose second stack is the head.
# pool / pool_backward: the op between the first and the second stack and its gradient.  centre_tap: the stem layers that
# are 1x1 in a `.weights` file and run 3x3 on their centre tap; narrow: (stem layer, filters in the file) of the layers
# that run wider than the file holds them, the padded filters and the next layer's padded input channels exactly zero.
# anchors: the published anchors of the graph.  wide: None, or (K, Cout) of the last convolution where it is wider than a
# stack's row and runs as engine.WideHead behind the head stack (a cfg under wide_head=True); the head stack then ends in
# an ordinary conv-BN-leaky layer, and the rules for a linear last layer do not apply to it.
_Topology = collections.namedtuple("_Topology", "name specs heights bn_eps slopes train_options head_statistics "
                                                "darknet_input concat concat_backward cf_stack pool pool_backward "
                                                "centre_tap narrow anchors wide", defaults=(None,))

_BESSEL = {"bessel": True}       # moving variances on the n - 1 estimate, as Darknet keeps them
_TOPOLOGY = {
    # (stem, 13x13 stack, head): the graph of the module docstring
    "paper": _Topology(name="paper", specs=yolov2_specs, heights=(32, 1, 1), bn_eps=None, slopes=(None, None, None),
                       train_options=({}, {}, {}), head_statistics=True, darknet_input=False, concat=_paper_concat,
                       concat_backward=E.passthrough_concat_backward, cf_stack=0, pool=E.max_pool_2x2,
                       pool_backward=E.max_pool_2x2_backward, centre_tap=(), narrow=(), anchors=ANCHORS_VOC),
    # (stem, 13x13 stack, route, head): the order of the convolutions in a `.weights` file.  The head trains its 3x3 layer
    # on batch statistics and runs the last, linear layer on its moving ones (core_layers 1)
    "darknet": _Topology(name="darknet", specs=yolov2_darknet_specs, heights=(32, 1, 2, 1), bn_eps=DARKNET_BN_EPS,
                         slopes=(None, None, None, [0.1, 1.0]),
                         train_options=(_BESSEL, _BESSEL, _BESSEL, dict(_BESSEL, core_layers=1)), head_statistics=False,
                         darknet_input=True, concat=E.passthrough_concat_darknet,
                         concat_backward=E.passthrough_concat_darknet_backward, cf_stack=2, pool=E.max_pool_2x2,
                         pool_backward=E.max_pool_2x2_backward, centre_tap=(DARKNET_1X1_CORE_LAYER,), narrow=(),
                         anchors=ANCHORS_VOC),
    # (stem, head): tiny-yolo-voc.cfg.  No passthrough; Darknet's stride-1 pool between the stacks; the "darknet" head with
    # one more core layer
    "tiny": _Topology(name="tiny", specs=yolov2_tiny_specs, heights=(32, 1), bn_eps=DARKNET_BN_EPS,
                      slopes=(None, [0.1, 0.1, 1.0]), train_options=(_BESSEL, dict(_BESSEL, core_layers=2)),
                      head_statistics=False, darknet_input=True, concat=None, concat_backward=None, cf_stack=None,
                      pool=E.max_pool_2x2_s1, pool_backward=E.max_pool_2x2_s1_backward, centre_tap=(),
                      narrow=TINY_NARROW, anchors=ANCHORS_TINY_VOC),
}


def _topology(name):
    if name not in TOPOLOGIES:
        raise ValueError("topology %r: one of %s" % (name, ", ".join(TOPOLOGIES)))
    return _TOPOLOGY[name]


def _cfg_topology(record, dtype, wide_head=False, training=False):
    """the _Topology of a Darknet cfg (utils/darknet_cfg.py) -> (topology, record): one more way to produce the record the
    code below reads, under the name of the shape it has -- "tiny" for a chain, "darknet" for a passthrough.  A cfg that
    describes yolov2-voc.cfg or tiny-yolo-voc.cfg gives the named topology's stacks, options and ops.  wide_head: the
    keyword of utils/darknet_cfg.py -- `map=` is admitted and a last convolution wider than a stack's row becomes the
    topology's `wide` operator; without it a record that carries `map` is refused here.  training: the caller is a
    trainer, and a wide head trains behind dtype 'f16' only"""
    from ..utils import darknet_cfg
    record = darknet_cfg.as_record(record, wide_head)
    if record.map is not None and not wide_head:
        raise ValueError("%s: map=%s: the class map of YOLO9000 belongs with its wide head; "
                         "from_cfg(..., wide_head=True) admits both" % (record.path, record.map))
    graph = darknet_cfg.compile_graph(record, 1024 if dtype == "f32" else darknet_cfg.MAX_OUT_WIDTH, wide_head)
    n, head = len(graph.specs), graph.head_layers
    wide = None
    if graph.wide:
        from .. import _lib
        if training and _lib.DTYPES.get(dtype, dtype) != _lib.Y2_F16:
            raise ValueError("%s: dtype %r with a wide head (%d filters): the wide head trains behind a model of dtype 'f16' "
                             "only -- its products round both operands to f16 under the stacks' loss scale%s" %
                             (record.path, dtype, graph.file_layers[-1][2],
                              ", and 'fp8' does not train anywhere" if dtype in ("fp8", "mxfp8") else ""))
        if _lib.DTYPES.get(dtype, dtype) not in (_lib.Y2_F16, _lib.Y2_FP8):
            raise ValueError("%s: dtype %r with a wide head (%d filters): the wide head has one arithmetic, f16 operands "
                             "with fp32 accumulation, and runs behind a model of dtype 'f16' or 'fp8' only -- the exact "
                             "modes exist for parity with the reference, which has no such layer" %
                             (record.path, dtype, graph.file_layers[-1][2]))
        wide = (graph.file_layers[-1][1], graph.file_layers[-1][2])
        slopes = (None,) * (n - 1) + ([0.1] * (head - 1),)                  # the head stack: conv-BN-leaky throughout
        options = (_BESSEL,) * n
    else:
        slopes = (None,) * (n - 1) + ([0.1] * (head - 1) + [1.0],)
        options = (_BESSEL,) * (n - 1) + (dict(_BESSEL, core_layers=head - 1),)
    common = dict(wide=wide, specs=lambda num_class, num_anchors, width_div, _s=graph.specs: tuple(list(s) for s in _s),
                  bn_eps=DARKNET_BN_EPS, slopes=slopes, train_options=options, head_statistics=False, darknet_input=True,
                  centre_tap=graph.centre_tap, narrow=graph.narrow, anchors=record.anchors)
    if graph.shape == "chain":
        s1 = graph.pool == "s1"
        topo = _Topology(name="tiny", heights=(32, 1), concat=None, concat_backward=None, cf_stack=None,
                         pool=E.max_pool_2x2_s1 if s1 else E.max_pool_2x2,
                         pool_backward=E.max_pool_2x2_s1_backward if s1 else E.max_pool_2x2_backward, **common)
    else:
        topo = _Topology(name="darknet", heights=(32, 1, 2, 1) if graph.route else (32, 1, 1),
                         concat=E.passthrough_concat_darknet, concat_backward=E.passthrough_concat_darknet_backward,
                         cf_stack=2 if graph.route else 0, pool=E.max_pool_2x2, pool_backward=E.max_pool_2x2_backward,
                         **common)
    return topo, record


def load_cfg_tree(record):
    """the word tree a cfg names (softmax_tree) -> a utils.word_tree.WordTree, or None where it names none.  The path is
    tried as written against the working directory, then against the cfg's directory; the tree must hold exactly the
    cfg's `classes` nodes"""
    import os
    from ..utils import word_tree
    if record.tree is None:
        return None
    tried = [record.tree, os.path.join(os.path.dirname(record.path), record.tree)]
    found = next((p for p in tried if os.path.isfile(p)), None)
    if found is None:
        raise ValueError("%s: softmax_tree=%s: no such file, neither %s nor %s" % (record.path, record.tree, tried[0],
                                                                                   tried[1]))
    tree = word_tree.load(found)
    if tree.n != record.classes:
        raise ValueError("%s: softmax_tree=%s holds %d nodes, classes=%d" % (record.path, record.tree, tree.n,
                                                                             record.classes))
    return tree


def _device_tree(tree, num_class, device):
    """tree: None, or a utils.word_tree.WordTree of num_class nodes -> its tables on the device"""
    if tree is None:
        return None
    if tree.n != num_class:
        raise ValueError("the word tree holds %d nodes, the model %d classes" % (tree.n, num_class))
    return E.WordTreeTables(tree, device)


def _build_stacks(topo, specs, batch, size, dtype, device, bn_eps, training, seed, share_with=None):
    """the stack contexts of one input size, in networks() order.  share_with: the contexts of another size, whose
    parameters these are bound to; without it every stack draws its initial values from seed + its position"""
    assert size % 32 == 0
    nets = []
    for i, (spec, units) in enumerate(zip(specs, topo.heights)):
        h = units * (size // 32)
        options = dict(topo.train_options[i], share_with=share_with[i] if share_with else None) if training else {}
        net = E.Network(spec, batch, h, h, dtype=dtype, training=training, device=device, **options)
        if topo.slopes[i] is not None or bn_eps is not None:
            net.set_layer_options(slopes=topo.slopes[i], bn_eps=bn_eps)
        if share_with is None:
            net.init_params(seed + i)
        nets.append(net)
    return tuple(nets)


def _make_buffers(topo, nets, batch, size):
    """(network input, concat) of one size on a topology that keeps them, else (None, None)"""
    if not topo.darknet_input:
        return None, None
    S, dev = size // 32, nets[0].device
    return (torch.empty((batch, size, size, 3), dtype=torch.float32, device=dev),
            torch.empty((batch, S, S, nets[-1].spec[0][1]), dtype=torch.float32, device=dev) if topo.concat else None)


def _forward(topo, nets, buffers, images, training, update_moving, out=None, wide=None):
    """the forward pass of every graph -> (flat head output, fine map).  nets = (stem, 13x13 stack, [route,] head), or
    (stem, head) on a graph without a passthrough.  wide: the engine.WideHead of a wide graph, run on the head stack's
    output"""
    x_buf, cat_buf = buffers
    if topo.darknet_input and images.dtype == torch.uint8:
        images = E.u8_to_darknet_input(images, out=x_buf)                   # BGR pixels -> RGB in [0, 1]
    stem, head = nets[0], nets[-1]
    fine = stem.forward(images, training, training, update_moving=update_moving)                  # [N,2S,2S,512]
    cat = topo.pool(fine)                                                   # "tiny": [N,S,S,512], the head's input
    if topo.concat is not None:
        coarse = nets[1].forward(cat, training, training, update_moving=update_moving)            # [N,S,S,1024]
        passed = fine
        for route in nets[2:-1]:                                            # "darknet": the 1x1 route, [N,2S,2S,64]
            passed = route.forward(passed, training, training, update_moving=update_moving)
        cat = topo.concat(passed, coarse, out=cat_buf)                      # [N,S,S,4*cf+1024], reorganised map first
    if wide is not None:                                                    # the head stack is an ordinary stack here
        return wide.forward(head.forward(cat, training, training, update_moving=update_moving), out=out), fine
    out = head.forward(cat, training, training and topo.head_statistics, out=out, update_moving=update_moving)
    return out, fine                                                        # [N,S,S,B*(5+C)]


class YOLOv2Detector:
    """topology "paper" (default): the graph of the module docstring.  "darknet": the graph of yolov2-voc.cfg, the one a
    Darknet `.weights` file holds (net_utils.load_darknet_weights / save_darknet_weights) -- a fourth stack, the 1x1
    route convolution 512 -> 64 on the fine map; Darknet's reorg (engine.passthrough_concat_darknet) with the
    reorganised map in FRONT of the 13x13 path; a last layer without activation; batch-norm epsilon 1e-6; and the input
    RGB in [0, 1]: uint8 BGR batches are converted by engine.u8_to_darknet_input, float input is taken as that already.
    "tiny": the graph of tiny-yolo-voc.cfg, Darknet's second VOC model (yolov2_tiny_specs; anchors ANCHORS_TINY_VOC) --
    two stacks with Darknet's stride-1 pool between them, no passthrough, the input, epsilon and last layer of "darknet".
    bn_eps: the batch-norm epsilon of every stack (None: the context's default 1e-3, or 1e-6 on "darknet" / "tiny").
    tree: a utils.word_tree.WordTree of num_class nodes (None: the flat softmax) -- a row's only class is then the node
    where the walk down the tree stops at tree_thresh, its score the objectness.  detect_batch and detect_tree_batch take
    the node from engine.word_tree_top and read no class row (detect_tree_batch); detect and detect_classes_batch
    rewrite the head through engine.word_tree_head (one launch between the forward pass and the rows)."""

    def __init__(self, batch, image_size=416, num_class=20, anchors=ANCHORS_VOC, dtype="f16", seed=0,
                 device="cuda:0", width_div=1, topology="paper", bn_eps=None, tree=None, tree_thresh=0.5, _cfg=None):
        assert image_size % 32 == 0
        # _cfg: (topology record, cfg record) of from_cfg -- the graph of a file under the name of its shape
        self._topo, self.cfg = _cfg if _cfg is not None else (_topology(topology), None)
        self.topology = topology = self._topo.name
        self.bn_eps = self._topo.bn_eps if bn_eps is None else float(bn_eps)
        self.batch, self.size, self.S = batch, image_size, image_size // 32
        self.num_class, self.anchors = num_class, np.asarray(anchors, np.float32).reshape(-1, 2)
        self.B, self.width_div = len(self.anchors), width_div
        self.iteration = 0                                   # of the snapshot last restored (net_utils)
        self.anchors_dev = torch.as_tensor(self.anchors).to(device).contiguous()
        self.tree, self.tree_thresh = _device_tree(tree, num_class, device), float(tree_thresh)
        specs = self._topo.specs(num_class, self.B, width_div)
        self._stacks = _build_stacks(self._topo, specs, batch, image_size, dtype, device, self.bn_eps, False, seed)
        self.stem, self.head = self._stacks[0], self._stacks[-1]
        if len(self._stacks) > 2:
            self.deep = self._stacks[1]
        if len(self._stacks) == 4:
            self.route = self._stacks[2]
        self._buffers = _make_buffers(self._topo, self._stacks, batch, image_size)
        # the wide last layer of a cfg under wide_head=True (engine.WideHead; None on every other model): filters drawn
        # from seed + the stack count, as a stack's would be, until net_utils.load_darknet_weights fills them
        self.wide = None
        if self._topo.wide is not None:
            K, Cout = self._topo.wide
            self.wide = E.WideHead(K, Cout, device)
            rng = np.random.default_rng(seed + len(self._stacks))
            self.wide.load(rng.standard_normal((K, Cout), np.float32) * np.float32(1.0 / np.sqrt(K)),
                           np.zeros(Cout, np.float32))

    @classmethod
    def from_cfg(cls, record_or_path, batch, image_size=None, dtype="f16", seed=0, device="cuda:0", tree=None,
                 tree_thresh=None, wide_head=False):
        """the detector of a Darknet cfg (utils/darknet_cfg.py: a record or a file): its graph, widths, class count and
        anchors, its word tree (load_cfg_tree) and tree_thresh; image_size defaults to the file's width; tree /
        tree_thresh: a caller's own in place of the file's.  net_utils.load_darknet_weights fills it from the `.weights`
        file that goes with the cfg.  wide_head=True admits YOLO9000's file: `map=` and a last layer wider than a stack's
        row, which runs as engine.WideHead (dtype 'f16' or 'fp8'; detect and detect_batch work as they are)"""
        topo, record = _cfg_topology(record_or_path, dtype, wide_head)
        return cls(batch, record.size if image_size is None else image_size, num_class=record.classes,
                   anchors=record.anchors, dtype=dtype, seed=seed, device=device,
                   tree=load_cfg_tree(record) if tree is None else tree,
                   tree_thresh=record.tree_thresh if tree_thresh is None else tree_thresh, _cfg=(topo, record))

    def networks(self):
        """the stack contexts: (stem, 13x13 stack, head), or on the "darknet" topology (stem, 13x13 stack, route, head)
        -- the order of the convolutions in a `.weights` file"""
        return self._stacks

    def forward(self, images, out=None):
        """images [N,size,size,3] fp32 (or uint8 BGR pixels) on the device -> raw grid [N,S,S,B,5+C] (in `out`, a
        contiguous fp32 tensor of that many elements, if given).  On the "darknet" topology fp32 input is RGB in [0, 1]"""
        out, _fine = _forward(self._topo, self._stacks, self._buffers, images, False, False, out=out, wide=self.wide)
        return out.view(self.batch, self.S, self.S, self.B, 5 + self.num_class)

    def _tree_head(self, grid, keep_raw=False):
        """the head the rows read: `grid` itself, or with a word tree its rewrite (in place unless keep_raw)"""
        if self.tree is None:
            return grid
        return E.word_tree_head(grid, self.tree, self.tree_thresh, out=None if keep_raw else grid)

    def detect(self, images, score_thresh=0.3, iou_thresh=0.45, max_out=100, class_aware=True):
        """-> boxes [N,K,4] (cx,cy,w,h relative), best score [N,K], class id [N,K], keep [N,max_out], count [N]"""
        grid = self._tree_head(self.forward(images))
        boxes, scores = E.decode_anchors(grid.contiguous(), self.anchors)
        best, cls = E.class_argmax(scores)
        keep, count = E.nms(boxes, best, cls, iou_thresh, score_thresh, max_out, class_aware)
        return boxes, best, cls, keep, count

    def detect_batch(self, images_u8, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_out=100, out=None,
                     grid_out=None, letterbox=False):
        """evaluation: images_u8 [N,size,size,3] uint8 BGR (DeviceVOC.eval_batch), table / index the pool's entry table
        and the slots' entries -> (det int32 [N,max_out,6], score [N,max_out], count [N]) in the 1-based pixels of each
        ORIGINAL image: the forward pass on the moving statistics, then ONE launch from the raw head
        (engine.detect_anchor_batch) -- rows that engine.voc_match_batch reads.  grid_out: keeps the raw head there.
        With a word tree and score_thresh >= 0 the same rows, bit for bit, come from detect_tree_batch (below a negative
        threshold, from the rewritten head: there a zero-score candidate's class is 0, not its node).
        letterbox: images_u8 is a letterboxed batch (DeviceVOC.eval_batch(..., letterbox=True)) and the boxes are
        un-mapped from each picture's rectangle."""
        if self.tree is not None and score_thresh >= 0:      # the same rows, bit for bit, without the rewrite
            return self.detect_tree_batch(images_u8, table, index, score_thresh, iou_thresh, max_out, out=out,
                                          grid_out=grid_out, letterbox=letterbox)
        grid = self._tree_head(self.forward(images_u8, out=grid_out), grid_out is not None)
        return E.detect_anchor_batch(grid, self.anchors_dev, table, index, score_thresh, iou_thresh, max_out, out=out,
                                     net_size=self.size if letterbox else None)

    def detect_tree_batch(self, images, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_out=100, out=None,
                          grid_out=None, letterbox=False, protocol="repo"):
        """detect_batch for a model with a word tree, from the tree's node instead of a class row (ValueError without a
        tree): the forward pass (into grid_out if given), engine.word_tree_top -- rows whose objectness does not pass
        score_thresh are not walked, where that is >= 0 -- and engine.detect_anchor_tree_batch: two launches behind the
        forward pass, the raw head left as it is, no rewritten tensor.  A candidate has one class, its node, so these
        class-aware rows are also what a per-class entry would return, at any width of the head.  protocol="darknet":
        Darknet's float rows for voc_match_batch_f, under detect_classes_batch's conditions (the "darknet" topology,
        letterbox=True, the float32 batch of DeviceVOC.eval_batch(..., protocol="darknet"))"""
        if self.tree is None:
            raise ValueError("detect_tree_batch needs a model with a word tree: a row's class is the tree's node")
        if protocol == "darknet":
            if not self._topo.darknet_input:
                raise ValueError("protocol='darknet' needs the \"darknet\" topology: the input of the %r topology is BGR "
                                 "in [-1, 1), not Darknet's RGB in [0, 1]" % (self.topology,))
            if not letterbox:
                raise ValueError("protocol='darknet' is letterboxed: pass letterbox=True")
            assert images.dtype == torch.float32, images.dtype
        elif protocol != "repo":
            raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
        grid = self.forward(images, out=grid_out)
        top, _prob = E.word_tree_top(grid, self.tree, self.tree_thresh, score_thresh if score_thresh >= 0 else None)
        return E.detect_anchor_tree_batch(grid, top, self.anchors_dev, table, index, score_thresh, iou_thresh, max_out,
                                          out=out, net_size=self.size if letterbox else None, protocol=protocol)

    def detect_classes_batch(self, images_u8, table, index=None, score_thresh=0.005, iou_thresh=0.45, max_per_class=32,
                             out=None, grid_out=None, letterbox=False, protocol="repo"):
        """detect_batch with one row per (candidate, class), as Darknet's `valid` scores a detector ->
        (det int32 [N,C,max_per_class,6], score [N,C,max_per_class], count [N,C]): engine.detect_anchor_classes_batch on
        the raw head.  protocol="darknet": the batch is the float32 RGB one of DeviceVOC.eval_batch(...,
        protocol="darknet") and the rows are Darknet's -- float un-map, float IoU, float corners as bit patterns in words
        0..3 (engine.detect_anchor_classes_batch_darknet).  It needs the "darknet" topology, whose float input is RGB in
        [0, 1], and letterbox=True"""
        if self.wide is not None:
            raise ValueError("detect_classes_batch on a model with a wide head (%d classes) is not built: it would launch "
                             "one workgroup per class and image, each re-deriving a %d-wide softmax; use detect_batch -- "
                             "with a word tree a row has one class, so its class-aware rows are the same detections" %
                             (self.num_class, self.num_class))
        if protocol == "darknet":
            if not self._topo.darknet_input:
                raise ValueError("protocol='darknet' needs the \"darknet\" topology: the input of the %r topology is BGR "
                                 "in [-1, 1), not Darknet's RGB in [0, 1]" % (self.topology,))
            if not letterbox:
                raise ValueError("protocol='darknet' is letterboxed: pass letterbox=True")
            assert images_u8.dtype == torch.float32, images_u8.dtype
            grid = self._tree_head(self.forward(images_u8, out=grid_out), grid_out is not None)
            return E.detect_anchor_classes_batch_darknet(grid, self.anchors_dev, table, index, score_thresh, iou_thresh,
                                                         max_per_class, out=out, net_size=self.size)
        if protocol != "repo":
            raise ValueError("protocol %r is neither 'repo' nor 'darknet'" % (protocol,))
        grid = self._tree_head(self.forward(images_u8, out=grid_out), grid_out is not None)
        return E.detect_anchor_classes_batch(grid, self.anchors_dev, table, index, score_thresh, iou_thresh,
                                             max_per_class, out=out, net_size=self.size if letterbox else None)


class _Trainer:
    """what the two train steps share: the contexts per input size on ONE set of parameters, the optimizers on one loss
    scaler, the gradient reducers, the step.  A subclass names its topology and adds what only it has."""

    keeps_backward = False           # whether backward() leaves last_dcat / last_dfine behind (a subclass's tests read them)

    def __init__(self, topology, batch, image_size, num_class, anchors, dtype, seed, device, scales, width_div,
                 area_weight, prior_images, prior_scale, solver, bn_eps, _cfg=None, tree=None, tree_thresh=0.5):
        self._topo, self.cfg = _cfg if _cfg is not None else (_topology(topology), None)
        # tree: a utils.word_tree.WordTree of num_class nodes (None: the flat softmax).  Box lists then train through
        # engine.yolov2_loss_boxes_tree, a truth's class a node index; tree_thresh is kept for the detector of this model
        self.tree, self.tree_thresh = _device_tree(tree, num_class, device), float(tree_thresh)
        topology = self._topo.name
        # the batch-norm epsilon of every context and size (None: the contexts' default, 1e-3); 1e-6 is Darknet's, the one
        # a backbone read from a Darknet file was trained with (net_utils.read_darknet_backbone)
        self.topology, self.bn_eps = topology, self._topo.bn_eps if bn_eps is None else float(bn_eps)
        from ..trainer import GradReducer
        self._GradReducer = GradReducer
        self.batch, self.num_class, self.dtype, self.device, self.seed = batch, num_class, dtype, device, seed
        self.anchors = np.asarray(anchors, np.float32)
        self.B, self.width_div = len(self.anchors), width_div
        self._anchors_dev = None                             # the anchors on the device, for step(stats=...)
        self.scales = scales
        # box-list labels only (step(images, truth=..., ntruth=...)): Darknet's (2 - w h) coord weight, and its anchor-prior
        # term while fewer than prior_images images have been seen ((iteration - 1) * batch, counted over resumed runs)
        self.area_weight, self.prior_images, self.prior_scale = bool(area_weight), int(prior_images), float(prior_scale)
        self.iteration = 0                                   # train steps taken, over resumed runs (net_utils snapshots)
        self.solver = solver.validate() if solver is not None else None
        self.specs = tuple(self._topo.specs(num_class, self.B, width_div))
        # the width the passthrough reorganises (None: a graph without one)
        self.cf = self.specs[self._topo.cf_stack][-1][2] if self._topo.cf_stack is not None else None
        self.ctx, self.reducers, self._buffers = {}, {}, {}
        self.opts = None
        self.default_size = image_size
        # the wide last layer of a cfg under wide_head=True (engine.WideHead; None on every other model), trained by Darknet's
        # solver as one more member of the joint step (engine.WideHeadSGD on the stacks' scaler)
        self.wide = self.wide_opt = None
        if self._topo.wide is not None:
            if self.solver is None:
                raise ValueError("a wide head (%d filters) trains under Darknet's solver only: pass solver= (Adam on the "
                                 "wide layer is not built)" % self._topo.wide[1])
            self._refuse_wide_replicas()
        self._nets(image_size)
        if self._topo.wide is not None:
            K, Cout = self._topo.wide
            self.wide = E.WideHead(K, Cout, device)
            rng = np.random.default_rng(seed + len(self.nets))             # as YOLOv2Detector draws them
            self.wide.load(rng.standard_normal((K, Cout), np.float32) * np.float32(1.0 / np.sqrt(K)),
                           np.zeros(Cout, np.float32))
            self.wide_opt = E.WideHeadSGD(self.wide, self.solver, self.opts[0].scaler)

    def _refuse_wide_replicas(self):
        from ..trainer import _dist
        dist = _dist()
        if dist is not None and dist.get_world_size() > 1:
            raise ValueError("a wide head does not train data parallel (world size %d): no reducer for its %d x %d filter "
                             "gradient is built" % (dist.get_world_size(), self._topo.wide[0], self._topo.wide[1]))

    def _nets(self, size):
        if size not in self.ctx:
            first = next(iter(self.ctx.values())) if self.ctx else None
            nets = _build_stacks(self._topo, self.specs, self.batch, size, self.dtype, self.device, self.bn_eps, True,
                                 self.seed, share_with=first)
            if first is None:
                self._init_form(nets)
                if self.solver is None:
                    self.opts = [E.AdamOptimizer(net) for net in nets]
                else:
                    self.opts = [E.DarknetSGD(net, self.solver) for net in nets]
                # ONE loss scale, overflow flag and step counter for the composed graph: an inf confined to
                # one stack must skip the step of all, and a skipped step must not advance any Adam bias correction
                for opt in self.opts[1:]:
                    opt.scaler = self.opts[0].scaler
            self.ctx[size] = nets
            self.reducers[size] = [self._GradReducer(net) for net in nets]
            self._buffers[size] = _make_buffers(self._topo, nets, self.batch, size)
        return self.ctx[size]

    def _init_form(self, nets):
        """bring a fresh model into the form its snapshots can hold (nothing to do here)"""

    def _mask_gradients(self, nets):
        """after the all-reduce, before the optimizers: zero the gradients that must not move (none here)"""

    @property
    def nets(self):
        return self.ctx[self.default_size]

    def networks(self, size=None):
        """the stack contexts of an input size: (stem, 13x13 stack, head), or on "darknet" (stem, 13x13 stack, route,
        head), the order of a `.weights` file"""
        return self._nets(size or self.default_size)

    def params_changed(self):
        """the shared parameters were written from outside (a file was loaded): every size's contexts re-pack"""
        for nets in self.ctx.values():
            for net in nets:
                net.params_changed()

    def forward(self, images, training=True, update_moving=False):
        """images [N,size,size,3] -> (raw grid [N,S,S,B,5+C], fine [N,2S,2S,Cf]).  "darknet": uint8 BGR pixels or fp32 RGB
        in [0, 1], and the last layer runs on its moving statistics in either mode"""
        size = int(images.shape[1])
        out, fine = _forward(self._topo, self._nets(size), self._buffers[size], images, training, update_moving,
                             wide=self.wide)
        return out.view(self.batch, size // 32, size // 32, self.B, 5 + self.num_class), fine

    def prior_on(self, iteration=None):
        """whether the anchor-prior term is part of train step `iteration` (1-based; default: the next one)"""
        i = self.iteration + 1 if iteration is None else int(iteration)
        return (i - 1) * self.batch < self.prior_images

    def box_scales(self, iteration=None):
        """the scale set of engine.yolov2_loss_boxes at a train step: `scales` + the area weight + the prior while on"""
        sc = dict(self.scales or {})
        sc["area_weight"] = 1.0 if self.area_weight else 0.0
        sc["prior_scale"] = self.prior_scale if self.prior_on(iteration) else 0.0
        return sc

    def backward(self, dnet, fine, size):
        """the whole backward pass of the forward(training) just run at `size`, from the head's output gradient `dnet`:
        gradients into the flat buffers, reduced over the replicas.  Returns the world size.  Each stack's all-reduce
        starts as soon as its gradients are complete and is joined after the stem's."""
        from ..trainer import _dist
        nets = self._nets(size)
        S = size // 32
        dist = _dist()
        red = self.reducers[size]
        dcat = nets[-1].backward_input(dnet.view(self.batch, S, S, -1))
        if dist is not None:
            red[-1].reduce_all_async()
        if self._topo.concat_backward is None:               # no passthrough: the pool's gradient is the fine map's
            dfine = self._topo.pool_backward(fine, dcat)
        else:
            dfine, dcoarse = self._topo.concat_backward(dcat, self.cf)
            dpooled = nets[1].backward_input(dcoarse)
            if dist is not None:
                red[1].reduce_all_async()
            for i in range(2, len(nets) - 1):                # "darknet": back through the route, to the fine map
                dfine = nets[i].backward_input(dfine)
                if dist is not None:
                    red[i].reduce_all_async()
            E.accumulate(dfine, self._topo.pool_backward(fine, dpooled))
        if self.keeps_backward:
            self.last_dcat, self.last_dfine = dcat, dfine
        world = red[0].backward_and_reduce(dfine)
        if dist is not None:
            for r in red[1:]:
                r.join()
        return world

    def step(self, images, labels=None, truth=None, ntruth=None, stats=None):
        """one train step on the label grid `labels` [N,S,S,5+C] (one box per cell) or on the box list `truth` [N,T,5] +
        `ntruth` [N] (every object; DeviceVOC(..., max_boxes=T)): exactly one of the two forms.  Returns loss[5] = coord,
        object, noobject, class, total.  stats: a six-float device tensor that engine.yolov2_region_stats fills from this
        step's head output, before the update (box lists only); None launches nothing more"""
        if (labels is None) == (truth is None) or (truth is None) != (ntruth is None):
            raise ValueError("step() takes either labels or truth + ntruth, not both and not neither")
        if stats is not None and truth is None:
            raise ValueError("step(stats=...) reads the box list: give truth + ntruth, not labels")
        if self.tree is not None and labels is not None:
            raise ValueError("a label grid with a word tree is not built: give the box list, truth + ntruth")
        size = int(images.shape[1])
        nets = self._nets(size)
        if len(self.ctx) > 1:
            for net in nets:
                net.params_changed()              # shared parameters moved under another size's contexts
        self.iteration += 1
        grid, fine = self.forward(images, True, update_moving=True)
        if labels is not None:
            loss, dnet = E.yolov2_loss(grid.contiguous(), labels, self.anchors, size, True, self.scales)
        elif self.tree is None:
            loss, dnet = E.yolov2_loss_boxes(grid.contiguous(), truth, ntruth, self.anchors, size, True,
                                             self.box_scales(self.iteration))
            if stats is not None:
                if self._anchors_dev is None:                # uploaded once: the statistics add two launches, no copy
                    self._anchors_dev = torch.as_tensor(self.anchors).to(grid.device).contiguous()
                E.yolov2_region_stats(grid.contiguous(), truth, ntruth, self._anchors_dev, size, out=stats)
        else:
            if self._anchors_dev is None:
                self._anchors_dev = torch.as_tensor(self.anchors).to(grid.device).contiguous()
            loss, dnet = E.yolov2_loss_boxes_tree(grid.contiguous(), truth, ntruth, self._anchors_dev, size, self.tree, True,
                                                  self.box_scales(self.iteration))
            if stats is not None:
                E.yolov2_region_stats_tree(grid.contiguous(), truth, ntruth, self._anchors_dev, size, self.tree, out=stats)
        self.last_dnet = dnet                                # the head's output gradient of this step (tests read it)
        scaler = self.opts[0].scaler
        if self.wide is not None:
            # the wide layer's gradients from the head stack's output of this pass, under the stacks' loss scale; what it
            # hands down is the head stack's output gradient (kept in last_wide_x / last_wide_dx: tests read them)
            self._refuse_wide_replicas()
            self.last_wide_x = nets[-1]._out
            dnet = self.last_wide_dx = self.wide.backward(self.last_wide_x, dnet, scaler.scale)
        world = self.backward(dnet, fine, size)
        for opt, net in zip(self.opts, nets):
            opt.net = net
            if scaler is not None:
                scaler.attach(net)
        if scaler is None:
            self._mask_gradients(nets)
            for opt in self.opts:
                opt.step(grad_mult=1.0 / world)
            return loss
        # every stack's sentinels into the one flag (on the gradients as the backward pass left them), the masks, then
        # the guarded updates: all of them or none
        for i, net in enumerate(nets):
            scaler.scan(net, more=(i > 0))
        if self.wide_opt is not None:
            self.wide_opt.scan()
        self._mask_gradients(nets)
        for i, opt in enumerate(self.opts):
            opt.step(grad_mult=1.0 / world, joint="first" if i == 0 else "next")
        if self.wide_opt is not None:
            self.wide_opt.step(grad_mult=1.0 / world, joint="next")
        return loss

    def flops_per_step(self, size=None, mfma_launches_only=False):
        """algorithmic FLOPs of one train step (3 x forward conv FLOPs, SURVEY 8(d) convention);
        mfma_launches_only: without the 3-channel first layer, which has its own (non-GEMM) kernels"""
        size = size or self.default_size
        tot = 0.0
        for spec, units in zip(self.specs, self._topo.heights):
            h = units * (size // 32)
            for (k, ci, co, pool) in spec:
                if not (mfma_launches_only and ci == 3):
                    tot += 2.0 * self.batch * h * h * k * k * ci * co
                if pool:
                    h = (h + 1) // 2
        return 3.0 * tot


class YOLOv2Trainer(_Trainer):
    """Train step of the YOLOv2 detector (NOT in the reference: its trainer is the YOLOv1 grid model).
    Three conv-BN-leaky stacks, each with its own flat parameter / gradient buffer and Adam state.  With `sizes`
    the input size may change from step to step (multi-scale {320..608}): one context + workspace per size, all
    bound to the same three parameter sets (engine.Network(share_with=...)).
    solver: None -- three engine.AdamOptimizer; a utils.solver.Solver -- three engine.DarknetSGD (momentum, weight decay
    on the filters, the burn-in / steps / poly rate schedule), again with ONE loss scaler, step counter and rate."""

    def __init__(self, batch, image_size=416, num_class=20, anchors=ANCHORS_VOC, dtype="f16", seed=0,
                 device="cuda:0", scales=None, width_div=1, area_weight=False, prior_images=0, prior_scale=0.01,
                 solver=None, bn_eps=None, topology="paper", tree=None, tree_thresh=0.5):
        if topology == "tiny":
            raise NotImplementedError("YOLOv2Trainer trains the paper topology only: the \"tiny\" graph needs Darknet's "
                                      "stride-1 pool and its gradient, zero-padded narrow layers and a last layer without "
                                      "batch statistics -- YOLOv2DarknetTrainer(topology=\"tiny\") has them")
        if topology != "paper":
            _topology(topology)
            raise NotImplementedError("YOLOv2Trainer trains the paper topology only: the %r graph needs the gradient of "
                                      "Darknet's reorg, a fourth optimizer and a last layer without batch statistics -- "
                                      "YOLOv2DarknetTrainer has them" % topology)
        _Trainer.__init__(self, topology, batch, image_size, num_class, anchors, dtype, seed, device, scales, width_div,
                          area_weight, prior_images, prior_scale, solver, bn_eps, tree=tree, tree_thresh=tree_thresh)


class YOLOv2DarknetTrainer(_Trainer):
    """Train step of the yolov2-voc.cfg graph (YOLOv2Detector(topology="darknet")): what a Darknet `.weights` file holds
    can be fine-tuned here and written back (net_utils.load_darknet_weights / load_darknet_prefix / save_darknet_weights
    take this object).  YOLOv2Trainer's constructor arguments and step() contract; FOUR stacks in file order -- stem,
    13x13 stack, the 1x1 route convolution, head -- each with its flat buffers, optimizer and gradient reducer, ONE loss
    scaler, step counter and rate; the multi-scale contexts share the four parameter sets.

    Differences from YOLOv2Trainer: Darknet's input (uint8 BGR batches through engine.u8_to_darknet_input; float input
    is RGB in [0, 1]); the route stack and Darknet's reorg (engine.passthrough_concat_darknet and its gradient, the
    reorganised map in FRONT); batch-norm epsilon 1e-6; moving variances on the n - 1 estimate (bessel; the
    normalisation itself stays on the biased variance: a known difference from Darknet); and a last layer that is
    linear and runs WITHOUT batch statistics -- the head context has core_layers = 1, its 1x1 layer normalises with the
    identity moving statistics the importer writes and its gamma / beta gradients are zeroed every step, so those four
    arrays never move and the export folds exactly 1.  The eight off-centre taps of core layer 3 (Darknet's 1x1) get a
    zero gradient every step too: they stay exactly zero and the model stays writable.
    backward() leaves the gradients at the concat and at the fine map in last_dcat / last_dfine (tests read them).

    topology="tiny": the graph of tiny-yolo-voc.cfg (YOLOv2Detector(topology="tiny"); pass anchors=ANCHORS_TINY_VOC for
    the published ones) under the same contract -- TWO stacks, Darknet's stride-1 pool and its gradient between them, a
    head with core_layers = 2.  Its first layer's filters 16 .. 31 and its second layer's input channels 16 .. 31 are the
    zero padding of yolov2_tiny_specs: a fresh model starts with them zero and their gradients (W, b, gamma, beta of the
    padded filters, W of the padded input channels) are zeroed every step, so they stay bit-zero under both optimizers,
    weight decay included, and the model stays writable.

    from_cfg(..., wide_head=True): a cfg whose last convolution is wider than a stack's row (YOLO9000's 28,269 filters).
    The head stack then ends in an ordinary conv-BN-leaky layer -- none of the last-layer rules above apply to it -- and the
    linear layer is `self.wide` (engine.WideHead), trained by `self.wide_opt` (engine.WideHeadSGD) as the last member of
    the joint step: dtype "f16", Darknet's solver, one process.  step() keeps the operator's input and the gradient it
    hands down in last_wide_x / last_wide_dx."""

    topology = "darknet"
    keeps_backward = True

    def __init__(self, batch, image_size=416, num_class=20, anchors=ANCHORS_VOC, dtype="f16", seed=0,
                 device="cuda:0", scales=None, width_div=1, area_weight=False, prior_images=0, prior_scale=0.01,
                 solver=None, bn_eps=None, topology="darknet", _cfg=None, tree=None, tree_thresh=0.5):
        if topology not in DARKNET_FILE_TOPOLOGIES:
            raise ValueError("YOLOv2DarknetTrainer trains the \"darknet\" and \"tiny\" topologies; topology %r is "
                             "YOLOv2Trainer's" % (topology,))
        _Trainer.__init__(self, topology, batch, image_size, num_class, anchors, dtype, seed, device, scales, width_div,
                          area_weight, prior_images, prior_scale, solver, bn_eps, _cfg=_cfg, tree=tree,
                          tree_thresh=tree_thresh)

    CFG_PRIOR_IMAGES = 12800         # Darknet's region layer hard-codes the prior's span and the (2 - w h) weight

    @classmethod
    def from_cfg(cls, record_or_path, batch=None, image_size=None, dtype="f16", seed=0, device="cuda:0", solver=None,
                 prior_images=None, tree=None, tree_thresh=None, wide_head=False):
        """the train step of a Darknet cfg (utils/darknet_cfg.py: a record or a file): its graph, widths, class count and
        anchors; its [net] solver; its [region] scales (coord_scale ... thresh); area_weight and prior_images 12800, which
        Darknet hard-codes; its word tree (load_cfg_tree) and tree_thresh.  batch and image_size default to the file's;
        solver / prior_images / tree / tree_thresh: a caller's own in place of the file's (a flag given on the command
        line).  wide_head=True admits YOLO9000's file: `map=` (kept unread) and a last layer wider than a stack's row,
        which trains as engine.WideHead under engine.WideHeadSGD -- dtype 'f16' only, one process only"""
        topo, record = _cfg_topology(record_or_path, dtype, wide_head, training=True)
        return cls(record.batch if batch is None else batch, record.size if image_size is None else image_size,
                   num_class=record.classes, anchors=record.anchors, dtype=dtype, seed=seed, device=device,
                   scales=dict(record.scales), area_weight=True,
                   prior_images=cls.CFG_PRIOR_IMAGES if prior_images is None else prior_images,
                   solver=record.solver if solver is None else solver, _cfg=(topo, record),
                   tree=load_cfg_tree(record) if tree is None else tree,
                   tree_thresh=record.tree_thresh if tree_thresh is None else tree_thresh)

    def _init_form(self, nets):
        """a fresh model in the form a `.weights` file can hold: the 1x1 layers' off-centre taps zero, the narrow layers'
        padding zero (utils/darknet_weights.pad_layer_params), the last layer's batch norm the importer's identity
        (utils/darknet_weights.to_layer_params)"""
        from ..utils import darknet_weights as dkw
        stem, head = nets[0], nets[-1]
        params = stem.export_params()
        for l in self._topo.centre_tap:
            W = params[l]["W"]
            centre = W[1, 1].copy()
            W[...] = 0
            W[1, 1] = centre
        for l, n_file in self._topo.narrow:
            k, ci, co, _pool = stem.spec[l]
            params[l] = dkw.pad_layer_params(dkw.strip_layer_params(params[l], ci, n_file, check=False), ci, co)
            co2 = stem.spec[l + 1][2]
            params[l + 1] = dkw.pad_layer_params(dkw.strip_layer_params(params[l + 1], n_file, co2, check=False), co, co2)
        stem.load_params(params)
        if self._topo.wide is not None:
            return                   # the head stack ends in an ordinary conv-BN-leaky layer: the linear layer is the operator
        params = head.export_params()
        n = params[-1]["b"].size
        params[-1].update(gamma=np.full(n, np.sqrt(1.0 + np.float64(self.bn_eps)), np.float32),
                          beta=np.zeros(n, np.float32), moving_mean=np.zeros(n, np.float32),
                          moving_var=np.ones(n, np.float32))
        head.load_params(params)

    def _mask_gradients(self, nets):
        """after the all-reduce, before the optimizers: no gradient for the eight off-centre taps of Darknet's 1x1 layers,
        for the zero padding of the narrow layers nor for the last layer's gamma / beta"""
        stem, head = nets[0], nets[-1]
        for l in self._topo.centre_tap:
            taps = stem.layer_views(l, grads=True)["W"].view(9, -1)
            E.zero_(taps[:4])
            E.zero_(taps[5:])
        for l, n_file in self._topo.narrow:
            g = stem.layer_views(l, grads=True)
            for row in g["W"].view(-1, g["W"].shape[3]):                  # [k k ci][co]: the padded filters of every row
                E.zero_(row[n_file:])
            for key in ("b", "gamma", "beta"):
                E.zero_(g[key][n_file:])
            for tap in stem.layer_views(l + 1, grads=True)["W"].flatten(0, 1):     # [k k][ci][co]: the padded inputs
                E.zero_(tap[n_file:])
        if self._topo.wide is not None:
            return                   # an ordinary last layer: its gamma and beta train
        g = head.layer_views(head.num_layers - 1, grads=True)
        E.zero_(g["gamma"])
        E.zero_(g["beta"])

    def resume_at(self, iteration):
        """continue a run whose `.weights` snapshot stood at `iteration` (seen // batch): the step count the prior term
        reads and, under Darknet's solver, the position in the rate schedule -- Darknet derives both from `seen`.  A
        `.weights` file carries no optimizer state: moments and the loss scale start afresh, as in Darknet"""
        self.iteration = int(iteration)
        if self.solver is not None:
            for opt in self.opts + ([self.wide_opt] if self.wide_opt is not None else []):
                opt.t = self.iteration
            scaler = self.opts[0].scaler
            if scaler is not None:
                c = scaler.ctrl.cpu()
                c[1] = self.iteration
                scaler.ctrl.copy_(c)
