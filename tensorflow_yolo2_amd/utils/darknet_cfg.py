"""Darknet's `.cfg` files for the YOLOv2 family (host only, no device): the parser, the immutable record a file becomes,
the graph the record compiles to, and `read_names` for the `.names` file that goes with it.

Grammar.  Sections are `[name]`, entries `key=value`; blank lines and lines starting with `#` or `;` are skipped;
whitespace around names, keys and values is ignored; a later duplicate key of one section wins, as in Darknet's option
list.  The first section is `[net]` or `[network]`; every later section is one Darknet layer, numbered from 0 in file
order.  `[route]` indices count in that numbering, a negative one relative to the route's own position.

Sections understood: `[convolutional]` (stride 1, pad 1, leaky or linear), `[maxpool]` (2 / 2 or 2 / 1), `[route]` (one or
two indices), `[reorg]` (stride 2) and a last `[region]` (coords 4, softmax 1, bias_match 1, rescore 1; `softmax_tree` or
its synonym `tree`, the path of a word-tree file as written -- utils/word_tree.py reads it, yolo2_nets/yolov2.py finds it
-- and `tree_thresh` in [0, 1); `map` is refused unless the caller passes wide_head=True: it belongs with YOLO9000's wide
head, see below).  Everything else
-- another section, another value, an unknown key of a section that is understood, a value that does not parse -- raises a
ValueError naming the file, the line, the layer and the item: a silently ignored key is how a model ends up trained
differently from what its file says.

`[net]`: width = height, a positive multiple of 32; channels 3; angle 0; batch; subdivisions (accepted: this trainer runs
the whole batch in one pass); the solver keys become a utils.solver.Solver through its own validate() -- `max_batches`
reaches the Solver under policy=poly only, where the rate reads it (the record keeps the file's value either way);
saturation, exposure and hue are the augmentation's.

Two graph shapes are accepted (`compile_graph`), the ones yolo2_nets/yolov2.py can run:
    chain        conv-BN-leaky layers with 2 / 2 pools, at most one 2 / 1 pool (it separates the stem from the head), five
                 stride-2 pools in all, a last convolution that is linear and has no batch norm ("tiny")
    passthrough  a stem ending in the fine map at stride 16, a 2 / 2 pool, the coarse stack, `[route]` back to the fine
                 map, an optional 1x1 conv-BN-leaky, `[reorg] stride=2`, `[route]` of the reorganised map and the last
                 coarse convolution in that order, the head ending in the linear convolution ("darknet")
Widths come from the file and are held to the executor's rules (y2_ctx_create): first layer 3 -> 32, inner input widths a
multiple of 32 and of 128 above 128, inner output widths a multiple of 32, at most 2048 outputs (1024 in fp32 storage).
The one padding device stays: a 16-filter first layer runs 32 wide.  Any other width is refused by layer, width and rule.

wide_head=True (parse, load, compile_graph; default False, under which nothing above changes) admits YOLO9000's file:
`map=FILE` is kept in the record's `map` as written and never opened (detection does not read it; the trainers refuse a
record that carries one), and the LAST convolution -- linear, no batch norm -- may be wider than the executor's row: the
graph is then `wide`, its head stack ends at the last conv-BN-leaky layer and the last convolution runs as
engine.WideHead behind it.  Its input width keeps the inner rules and every batch-norm layer keeps the row limit."""
import collections

import numpy as np

from .darknet_weights import layer_floats
from .solver import Solver

Layer = collections.namedtuple("Layer", "index line kind options")       # options: a tuple of (key, value) pairs
Augmentation = collections.namedtuple("Augmentation", "jitter hue saturation exposure")

# the record of one file.  layers: the Layer tuple in file order (without [net]); solver: the utils.solver.Solver;
# augmentation: jitter (of [region]) and hue / saturation / exposure (of [net]); anchors: ((w, h), ...) in cells of stride
# 32; scales: ((name, value), ...) of coord_scale, object_scale, noobject_scale, class_scale, thresh; size, batch,
# subdivisions, max_batches, random: of [net] / [region]; file_layers: [(k, c, n, batch_norm)] in file order, the form
# utils/darknet_weights.split takes; floats: their float count; tree: softmax_tree as written (None: no word tree);
# tree_thresh: where a detection's walk down the tree stops (0.5 when absent, the default of Darknet's -hier); map: `map=`
# as written (None: absent; read under wide_head=True only, never opened)
DarknetCfg = collections.namedtuple("DarknetCfg", "path layers solver augmentation anchors classes num scales size batch "
                                                  "subdivisions max_batches random file_layers floats tree tree_thresh map",
                                    defaults=(None, 0.5, None))

# what compile_graph returns: shape "chain" / "passthrough"; specs: the stacks in networks() order, each a tuple of
# (k, in, out, pool) at the widths that RUN; file_layers as above; centre_tap: the stem layers that are 1x1 in the file
# and run 3x3 on their centre tap; narrow: ((stem layer, filters in the file), ...); head_layers: convolutions of the
# head; pool: "s2" / "s1", the op between the stem and the next stack; route: whether the passthrough has its convolution;
# wide: the last convolution is wider than max_out and is NOT part of the head stack's spec (engine.WideHead runs it);
# head_layers counts it all the same
Graph = collections.namedtuple("Graph", "shape specs file_layers centre_tap narrow head_layers pool route wide",
                               defaults=(False,))

SCALE_KEYS = ("coord_scale", "object_scale", "noobject_scale", "class_scale", "thresh")
MAX_OUT_WIDTH = 2048             # the batch-norm kernels' row width in 16-bit storage; fp32 storage: 1024
CENTRE_TAP_POOLS = 2             # a 1x1 convolution behind at most this many pools runs 3x3 on its centre tap


class _Fail(object):
    """the one error form: file:line: layer: item"""

    def __init__(self, path):
        self.path = path

    def __call__(self, line, where, what):
        raise ValueError("%s:%d: %s: %s" % (self.path, line, where, what))


def _where(index, kind):
    return "[%s]" % kind if index is None else "layer %d [%s]" % (index, kind)


def _sections(text, fail):
    """-> [(name, line, {key: (value, line)})] in file order"""
    out = []
    for no, raw in enumerate(text.splitlines(), 1):
        s = raw.strip()
        if not s or s[0] in "#;":
            continue
        if s[0] == "[":
            if s[-1] != "]" or not s[1:-1].strip():
                fail(no, "section", "%r is no [name]" % s)
            out.append((s[1:-1].strip(), no, {}))
            continue
        if "=" not in s:
            fail(no, _where(len(out) - 2 if len(out) > 1 else None, out[-1][0]) if out else "before the first section",
                 "%r is neither a [section] nor key=value" % s)
        if not out:
            fail(no, "before the first section", "%r stands in front of [net]" % s)
        key, value = s.split("=", 1)
        out[-1][2][key.strip()] = (value.strip(), no)
    return out


class _Options(object):
    """the options of one section: every read key is ticked off, done() refuses what is left"""

    def __init__(self, fail, index, kind, line, entries):
        self.fail, self.where, self.line, self.entries = fail, _where(index, kind), line, dict(entries)
        self.seen, self.lines = [], {}                           # (key, value) pairs read; the line of each

    def _parse(self, key, default, parse, what):
        if key not in self.entries:
            if default is _REQUIRED:
                self.fail(self.line, self.where, "%s is missing" % key)
            return default
        value, line = self.entries.pop(key)
        try:
            v = parse(value)
        except ValueError:
            self.fail(line, self.where, "%s=%s is no %s" % (key, value, what))
        self.seen.append((key, v))
        self.lines[key] = line
        return v

    def line_of(self, key):
        """the line a key stands on, or the section's where the key is absent"""
        return self.lines.get(key, self.line)

    def int(self, key, default):
        return self._parse(key, default, int, "integer")

    def float(self, key, default):
        def finite(s):
            v = float(s)
            if not np.isfinite(v):
                raise ValueError(s)
            return v
        return self._parse(key, default, finite, "number")

    def word(self, key, default):
        return self._parse(key, default, str, "word")

    def ints(self, key, default):
        return self._parse(key, default, lambda s: tuple(int(v) for v in s.split(",") if v.strip()), "list of integers")

    def floats(self, key, default):
        return self._parse(key, default, lambda s: tuple(float(v) for v in s.split(",") if v.strip()), "list of numbers")

    def must(self, key, value, allowed, why):
        if value not in allowed:
            self.fail(self.line_of(key), self.where, "%s=%s: %s" % (key, value, why))
        return value

    def done(self):
        for key, (value, line) in sorted(self.entries.items(), key=lambda kv: kv[1][1]):
            self.fail(line, self.where, "unknown key %s=%s" % (key, value))
        return tuple(self.seen)


_REQUIRED = object()
REFUSED_REGION_KEYS = ("map",)


def _parse_net(o):
    width, height = o.int("width", _REQUIRED), o.int("height", _REQUIRED)
    if height != width:
        o.fail(o.line_of("height"), o.where, "height=%d is not width=%d: the detector's input is square" % (height, width))
    if width < 32 or width % 32:
        o.fail(o.line_of("width"), o.where, "width=%d: a positive multiple of 32" % width)
    o.must("channels", o.int("channels", 3), (3,), "the first layer reads 3 channels")
    batch, subdivisions = o.int("batch", 1), o.int("subdivisions", 1)
    if batch < 1:
        o.fail(o.line_of("batch"), o.where, "batch=%d: at least 1" % batch)
    if subdivisions < 1:
        o.fail(o.line_of("subdivisions"), o.where, "subdivisions=%d: at least 1" % subdivisions)
    angle = o.float("angle", 0.0)
    o.must("angle", angle, (0.0,), "rotation is not built")
    power = o.float("power", 4.0)
    if power != int(power):
        o.fail(o.line_of("power"), o.where, "power=%s: the solver takes an integer exponent" % power)
    policy = o.word("policy", "constant")
    max_batches = o.int("max_batches", 0)
    fields = dict(learning_rate=o.float("learning_rate", 0.001), momentum=o.float("momentum", 0.9),
                  decay=o.float("decay", 0.0001), policy=policy, burn_in=o.int("burn_in", 0), power=int(power),
                  steps=o.ints("steps", ()), scales=o.floats("scales", ()),
                  max_batches=max_batches if policy == "poly" else 0)
    try:
        solver = Solver(**fields)
    except ValueError as e:
        key = str(e).split(" ", 1)[0]
        o.fail(o.line_of(key), o.where, "%s" % e)
    colour = (o.float("hue", 0.0), o.float("saturation", 1.0), o.float("exposure", 1.0))
    o.done()
    return dict(size=width, batch=batch, subdivisions=subdivisions, max_batches=max_batches, solver=solver, colour=colour)


def _parse_region(o, wide_head=False):
    for key in REFUSED_REGION_KEYS:
        if key in o.entries and not wide_head:
            o.fail(o.entries[key][1], o.where, "%s=%s: the class map of YOLO9000 belongs with its 28,269-wide head and is "
                   "not built" % (key, o.entries[key][0]))
    classes, num = o.int("classes", 20), o.int("num", 1)
    if classes < 1 or num < 1:
        o.fail(o.line, o.where, "classes=%d, num=%d: both at least 1" % (classes, num))
    anchors = o.floats("anchors", _REQUIRED)
    if len(anchors) != 2 * num:
        o.fail(o.line_of("anchors"), o.where, "anchors holds %d numbers, num=%d needs %d" % (len(anchors), num, 2 * num))
    if any(not (np.isfinite(a) and a > 0) for a in anchors):
        o.fail(o.line_of("anchors"), o.where, "anchors %s: each finite and > 0" % (anchors,))
    o.must("coords", o.int("coords", 4), (4,), "a box has 4 coordinates")
    o.must("softmax", o.int("softmax", 0), (1,), "the loss is the softmax one (softmax=1)")
    o.must("bias_match", o.int("bias_match", 0), (1,), "the loss matches truths to anchors by shape (bias_match=1)")
    o.must("rescore", o.int("rescore", 0), (1,), "the object target is the IoU (rescore=1); rescore=0 is not built")
    random = o.must("random", o.int("random", 0), (0, 1), "0 or 1")
    o.int("absolute", 0)                                      # accepted, not used
    scales = tuple((k, o.float(k, 0.5 if k == "thresh" else 1.0)) for k in SCALE_KEYS)
    jitter = o.float("jitter", 0.2)
    tree, tree_key = o.word("softmax_tree", None), "softmax_tree"
    synonym = o.word("tree", None)                            # the key YOLO9000's cfg writes
    if synonym is not None:
        if tree is not None and tree != synonym:
            o.fail(o.line_of("tree"), o.where, "tree=%s and softmax_tree=%s name different files" % (synonym, tree))
        tree, tree_key = synonym, "tree"
    if tree is not None and not tree:
        o.fail(o.line_of(tree_key), o.where, "%s= names no file" % tree_key)
    class_map = o.word("map", None) if wide_head else None
    if class_map is not None and not class_map:
        o.fail(o.line_of("map"), o.where, "map= names no file")
    tree_thresh = o.float("tree_thresh", 0.5)
    if not 0.0 <= tree_thresh < 1.0:
        o.fail(o.line_of("tree_thresh"), o.where, "tree_thresh=%s: a number in [0, 1)" % tree_thresh)
    o.done()
    return dict(classes=classes, num=num, anchors=tuple(zip(anchors[0::2], anchors[1::2])), random=random, scales=scales,
                jitter=jitter, tree=tree, tree_thresh=tree_thresh, map=class_map)


def _parse_layer(o, kind, index, fail):
    """-> the Layer options of one section (validated)"""
    if kind == "convolutional":
        bn = o.must("batch_normalize", o.int("batch_normalize", 0), (0, 1), "0 or 1")
        filters, size = o.int("filters", _REQUIRED), o.int("size", _REQUIRED)
        if filters < 1:
            o.fail(o.line_of("filters"), o.where, "filters=%d: at least 1" % filters)
        o.must("size", size, (1, 3), "1x1 and 3x3 convolutions exist")
        o.must("stride", o.int("stride", 1), (1,), "convolutions run at stride 1")
        o.must("pad", o.int("pad", 0), (1,), "convolutions pad by size / 2 (pad=1)")
        act = o.must("activation", o.word("activation", "logistic"), ("leaky", "linear"), "leaky or linear")
        o.done()
        return (("batch_normalize", bn), ("filters", filters), ("size", size), ("activation", act))
    if kind == "maxpool":
        size, stride = o.int("size", _REQUIRED), o.int("stride", _REQUIRED)
        o.must("size", size, (2,), "pools are 2 wide")
        o.must("stride", stride, (1, 2), "size 2 with stride 2 or stride 1")
        o.done()
        return (("size", size), ("stride", stride))
    if kind == "route":
        layers = o.ints("layers", _REQUIRED)
        if not 1 <= len(layers) <= 2:
            o.fail(o.line_of("layers"), o.where, "layers=%s: one or two indices" % ",".join(str(v) for v in layers))
        resolved = tuple(v if v >= 0 else index + v for v in layers)
        if any(not 0 <= v < index for v in resolved):
            o.fail(o.line_of("layers"), o.where, "layers=%s: every index must name an earlier layer" %
                   ",".join(str(v) for v in layers))
        o.done()
        return (("layers", resolved),)
    if kind == "reorg":
        o.must("stride", o.int("stride", 1), (2,), "the passthrough reorganises by 2")
        o.done()
        return (("stride", 2),)
    fail(o.line, o.where, "section [%s] is not understood ([convolutional], [maxpool], [route], [reorg], [region])" % kind)


def parse(text, path="<cfg>", wide_head=False):
    """the text of a cfg -> DarknetCfg; `path` is the name the errors carry; wide_head: admit `map=` and a last
    convolution wider than the executor's row (the module docstring)"""
    fail = _Fail(path)
    sections = _sections(text, fail)
    if not sections or sections[0][0] not in ("net", "network"):
        fail(sections[0][1] if sections else 1, "first section", "it must be [net] or [network]%s" %
             (", not [%s]" % sections[0][0] if sections else ""))
    name, line, entries = sections[0]
    net = _parse_net(_Options(fail, None, name, line, entries))
    layers, region = [], None
    for index, (kind, line, entries) in enumerate(sections[1:]):
        o = _Options(fail, index, kind, line, entries)
        if kind == "region":
            if index != len(sections) - 2:
                fail(line, o.where, "[region] must be the last section; %d follow(s)" % (len(sections) - 2 - index))
            region = _parse_region(o, wide_head)
            layers.append(Layer(index, line, kind, ()))
        else:
            layers.append(Layer(index, line, kind, _parse_layer(o, kind, index, fail)))
    if region is None:
        fail(sections[-1][1], _where(len(sections) - 2 if len(sections) > 1 else None, sections[-1][0]),
             "the last section must be [region]")
    hue, saturation, exposure = net["colour"]
    partial = DarknetCfg(path=path, layers=tuple(layers), solver=net["solver"],
                         augmentation=Augmentation(region["jitter"], hue, saturation, exposure), anchors=region["anchors"],
                         classes=region["classes"], num=region["num"], scales=region["scales"], size=net["size"],
                         batch=net["batch"], subdivisions=net["subdivisions"], max_batches=net["max_batches"],
                         random=region["random"], file_layers=(), floats=0, tree=region["tree"],
                         tree_thresh=region["tree_thresh"], map=region["map"])
    graph = compile_graph(partial, wide_head=wide_head)
    return partial._replace(file_layers=graph.file_layers, floats=sum(layer_floats(l) for l in graph.file_layers))


def load(path, wide_head=False):
    """a cfg file -> DarknetCfg"""
    with open(path, "r") as f:
        return parse(f.read(), str(path), wide_head)


def load_graph(path, max_out=MAX_OUT_WIDTH):
    """a cfg file -> (DarknetCfg, Graph, wide_head) for a caller that takes either kind of file: read under the default
    keyword where that succeeds; else under wide_head=True, and only where the graph then IS wide -- every other file keeps
    the refusal the default keyword gives it (a `map=` on a narrow model, a width the executor does not run)"""
    try:
        record = load(path)
        return record, compile_graph(record, max_out), False
    except ValueError as refusal:
        try:
            record = load(path, True)
            graph = compile_graph(record, max_out, True)
        except ValueError:
            raise refusal
        if not graph.wide:
            raise refusal
        return record, graph, True


def as_record(record_or_path, wide_head=False):
    return record_or_path if isinstance(record_or_path, DarknetCfg) else load(record_or_path, wide_head)


def read_names(path):
    """a `.names` file -> the class names, one per non-empty line"""
    with open(path, "r") as f:
        return [line.strip() for line in f.read().splitlines() if line.strip()]


# ---------------------------------------------------------------------------
# From the layer list to the stacks
# ---------------------------------------------------------------------------
def _check_widths(fail, convs, stack, max_out, wide=False):
    """the executor's rules on one stack's (layer, k, in, out, pool) rows at the widths that run; wide: the last
    convolution of the file is engine.WideHead's and has no output limit here"""
    for (layer, _k, ci, co, _pool) in stack:
        where = _where(layer.index, layer.kind)
        inner_in = not (layer is convs[0])
        if inner_in and ci % 32:
            fail(layer.line, where, "input width %d: an inner layer's input width must be a multiple of 32" % ci)
        if inner_in and ci > 128 and ci % 128:
            fail(layer.line, where, "input width %d: an input width above 128 must be a multiple of 128" % ci)
        if layer is not convs[-1] and co % 32:
            fail(layer.line, where, "width %d (filters): an inner layer's output width must be a multiple of 32" % co)
        if co > max_out and not (wide and layer is convs[-1]):
            fail(layer.line, where, "width %d (filters): at most %d outputs%s" %
                 (co, max_out, " in fp32 storage" if max_out < MAX_OUT_WIDTH else ""))


def compile_graph(record, max_out=MAX_OUT_WIDTH, wide_head=False):
    """the layer list of a record -> Graph, or ValueError naming the layer that fits neither shape or breaks a width rule.
    max_out: the widest output the executor runs (2048; 1024 where the tensors are stored in fp32).  wide_head: a last
    convolution above max_out is allowed and makes the graph `wide`"""
    fail = _Fail(record.path)
    layers = record.layers
    opt = lambda layer: dict(layer.options)
    body = layers[:-1]
    convs = [l for l in body if l.kind == "convolutional"]
    if len(convs) < 3:
        fail(layers[-1].line, _where(layers[-1].index, "region"), "the graph needs at least three convolutions")
    for l in convs[:-1]:
        if not (opt(l)["batch_normalize"] == 1 and opt(l)["activation"] == "leaky"):
            fail(l.line, _where(l.index, l.kind), "every convolution but the last is batch_normalize=1, activation=leaky")
    last = convs[-1]
    if last is not body[-1] or opt(last)["batch_normalize"] != 0 or opt(last)["activation"] != "linear":
        fail(body[-1].line, _where(body[-1].index, body[-1].kind),
             "the section in front of [region] must be a convolution with activation=linear and no batch norm")
    want = record.num * (5 + record.classes)
    if opt(last)["filters"] != want:
        fail(last.line, _where(last.index, last.kind), "filters=%d: num (5 + classes) = %d (%d + 5) = %d" %
             (opt(last)["filters"], record.num, record.classes, want))
    wide = bool(wide_head) and want > max_out
    if wide and opt(last)["size"] != 1:
        fail(last.line, _where(last.index, last.kind), "size=%d: a last convolution of %d filters runs as the wide head, "
             "which is 1x1" % (opt(last)["size"], want))
    first = convs[0]
    if first is not body[0] or opt(first)["size"] != 3 or opt(first)["filters"] not in (16, 32):
        fail(body[0].line, _where(body[0].index, body[0].kind), "the first layer must be a 3x3 convolution of 32 filters "
             "(or 16, which run 32 wide): filters=%s" % (opt(body[0]).get("filters"),))
    routes = [l for l in body if l.kind == "route"]
    shape = "passthrough" if routes or any(l.kind == "reorg" for l in body) else "chain"

    # walk the sections into segments of (layer, k, in, out, pool) rows; `width` is the file's, `run` the stack's
    narrow = ((0, 16),) if opt(first)["filters"] == 16 else ()
    segments, rows = [], []
    file_layers, centre_tap = [], []
    width_file = width_run = 3
    pools = 0                      # stride-2 pools seen
    out_of = {}                    # layer index -> (file width, run width) of its output
    s1_at = None

    def conv_row(l, cin_file, cin_run):
        o = opt(l)
        n_file = o["filters"]
        n_run = 32 if (l is first and narrow) else n_file
        k = o["size"]
        file_layers.append((k, cin_file, n_file, bool(o["batch_normalize"])))
        if k == 1 and not segments and pools <= CENTRE_TAP_POOLS:
            centre_tap.append(len(rows))
            k = 3
        rows.append([l, k, cin_run, n_run, 0])
        return n_file, n_run

    i = 0
    state = "stem"                 # passthrough: stem -> deep -> route -> head
    fine = None
    while i < len(body):
        l = body[i]
        where = _where(l.index, l.kind)
        if l.kind == "convolutional":
            width_file, width_run = conv_row(l, width_file, width_run)
            out_of[l.index] = (width_file, width_run)
        elif l.kind == "maxpool":
            stride = opt(l)["stride"]
            if not rows or body[i - 1].kind != "convolutional":
                fail(l.line, where, "a pool must follow a convolution")
            if state != "stem":
                fail(l.line, where, "a pool behind the %s: pools belong to the stem" %
                     ("2 / 1 pool" if shape == "chain" else "fifth stride-2 pool"))
            if stride == 1:
                if shape != "chain":
                    fail(l.line, where, "a 2 / 1 pool in a graph with a passthrough is not built")
                if pools != 5:
                    fail(l.line, where, "the 2 / 1 pool stands behind %d stride-2 pools: all five come first" % pools)
                s1_at = l.index
                segments.append(rows)
                rows, state = [], "head"
            else:
                pools += 1
                if pools > 5:
                    fail(l.line, where, "a sixth stride-2 pool: the head runs at stride 32")
                if shape == "passthrough" and pools == 5:
                    fine = body[i - 1]
                    segments.append(rows)
                    rows, state = [], "deep"
                else:
                    rows[-1][4] = 1
            out_of[l.index] = (width_file, width_run)
        elif l.kind == "route":
            targets = opt(l)["layers"]
            if state == "deep" and len(targets) == 1:
                if fine is None or targets[0] != fine.index:
                    fail(l.line, where, "layers=%d: the passthrough routes back to the fine map, layer %d (the convolution "
                         "in front of the fifth pool)" % (targets[0], fine.index if fine is not None else -1))
                if not rows:
                    fail(l.line, where, "no convolution between the fifth pool and the route")
                coarse = body[i - 1]
                if coarse.kind != "convolutional":
                    fail(l.line, where, "the route must follow the last coarse convolution")
                segments.append(rows)
                rows, state = [], "route"
                width_file, width_run = out_of[fine.index]
                j = i + 1
                if j < len(body) and body[j].kind == "convolutional":
                    if opt(body[j])["size"] != 1:
                        fail(body[j].line, _where(body[j].index, body[j].kind), "size=%d: the convolution on the route is "
                             "1x1" % opt(body[j])["size"])
                    width_file, width_run = conv_row(body[j], width_file, width_run)
                    out_of[body[j].index] = (width_file, width_run)
                    j += 1
                at = body[min(j, len(body) - 1)]            # where an error points: the section that is not what follows
                if j >= len(body) or body[j].kind != "reorg":
                    fail(at.line, _where(at.index, at.kind), "[reorg] must follow the route to the fine map (and its "
                         "optional 1x1 convolution)")
                reorg = body[j]
                j += 1
                at = body[min(j, len(body) - 1)]
                if j >= len(body) or body[j].kind != "route" or opt(body[j])["layers"] != (reorg.index, coarse.index):
                    fail(at.line, _where(at.index, at.kind), "behind [reorg] comes a [route] of layers %d and %d, in that "
                         "order: the reorganised map, then the last coarse convolution" % (reorg.index, coarse.index))
                cf_file, cf_run = width_file, width_run
                width_file = 4 * cf_file + out_of[coarse.index][0]
                width_run = 4 * cf_run + out_of[coarse.index][1]
                segments.append(rows)          # the route stack: zero or one layer
                rows, state = [], "head"
                i = j
            else:
                fail(l.line, where, "layers=%s: the one route shape built is the passthrough (back to the fine map, then "
                     "the reorganised map with the last coarse convolution)" % ",".join(str(v) for v in targets))
        elif l.kind == "reorg":
            fail(l.line, where, "[reorg] without the route to the fine map in front of it")
        i += 1
    segments.append(rows)
    if shape == "chain":
        if s1_at is None:
            # no 2 / 1 pool: the fifth stride-2 pool separates the stem from the head
            if pools != 5:
                fail(layers[-1].line, _where(layers[-1].index, "region"), "%d stride-2 pools: the head runs at stride 32, "
                     "five pools" % pools)
            rows = segments[0]
            cut = max(p for p, r in enumerate(rows) if r[4] == 1)
            rows[cut][4] = 0
            segments = [rows[:cut + 1], rows[cut + 1:]]
            centre_tap = [p for p in centre_tap if p <= cut]
            for r in segments[1]:      # behind the cut nothing is a centre tap: the file's filter size runs
                r[1] = dict(r[0].options)["size"]
        pool = "s1" if s1_at is not None else "s2"
        if len(segments) != 2:
            fail(layers[-1].line, _where(layers[-1].index, "region"), "the chain has no head behind its last pool")
    else:
        pool = "s2"
        if state != "head" or len(segments) != 4:
            fail(layers[-1].line, _where(layers[-1].index, "region"), "the passthrough is incomplete: stem, fifth pool, "
                 "coarse stack, route, [reorg], route, head")
        if not segments[2]:
            segments = [segments[0], segments[1], segments[3]]
    head = segments[-1]
    if len(head) < 2:
        at = head[0][0] if head else layers[-1]
        fail(at.line, _where(at.index, at.kind), "the head needs a conv-BN-leaky layer in front of the linear convolution")
    for stack in segments:
        if not stack:
            fail(layers[-1].line, _where(layers[-1].index, "region"), "a stack of the graph holds no convolution")
        if stack is not segments[0] and any(r[4] for r in stack):
            fail(stack[0][0].line, _where(stack[0][0].index, stack[0][0].kind), "pools belong to the stem")
        _check_widths(fail, convs, stack, max_out, wide)
    if narrow and len(segments[0]) < 2:
        fail(first.line, _where(first.index, first.kind), "a 16-filter first layer needs a second stem layer behind it")
    n_head = len(head)
    if wide:
        segments = segments[:-1] + [head[:-1]]     # the head stack ends at the last conv-BN-leaky layer
    specs = tuple(tuple((k, ci, co, p) for (_l, k, ci, co, p) in stack) for stack in segments)
    return Graph(shape=shape, specs=specs, file_layers=tuple(file_layers), centre_tap=tuple(centre_tap), narrow=narrow,
                 head_layers=n_head, pool=pool, route=(shape == "passthrough" and len(segments) == 4), wide=wide)
