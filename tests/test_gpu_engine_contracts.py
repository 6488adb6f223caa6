"""The contracts engine.py states once (its private helpers) as its public functions show them: a caller's `out` tensors
come back by identity, views of the right element count are accepted where the rows are checked by count and refused
where the shape is exact, every malformed tensor is an AssertionError before any launch, the ValueError and
y2_last_error texts are the documented ones, anchors may be a list, an array or a device tensor, and the three
flat-buffer optimizers export, load and step as their shared base says.  The values themselves are pinned bit for bit
against the numpy specifications by the test files of each kernel; here the smallest shapes that reach every branch:
one head of n = 2, S = 2, B = 2, C = 3 at net_size 64, a pool of two tiny images, max_out 4, max_per_class 2."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_gpu_sgd_solver import SPEC, N as BATCH, SIZE
from tensorflow_yolo2_amd.utils import solver as S

pytestmark = pytest.mark.gpu

n, GRID, B, NCLS, NET_SIZE, MAX_OUT, PER_CLASS, CANVAS = 2, 2, 2, 3, 64, 4, 2, 32
ANCHORS = ((1.3221, 1.73145), (3.19275, 4.00944))
ANCHOR_DETECTS = ("detect_anchor_batch", "detect_anchor_classes_batch", "detect_anchor_classes_batch_darknet")
ANCHOR_ENTRIES = ("y2_detect_anchor_batch", "y2_detect_anchor_batch_lb", "y2_detect_anchor_classes_batch",
                  "y2_detect_anchor_classes_batch_lb", "y2_detect_anchor_classes_batch_dk")
NINE = ("detect_grid_batch", "letterbox_batch", "warp_batch", "letterbox_darknet_batch", "voc_match_batch",
        "voc_match_batch_f") + ANCHOR_DETECTS


def _cuda(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


class Kit:
    """the inputs every test shares, made once and left unchanged, and one call of each of the nine wrappers"""

    def __init__(self):
        from tensorflow_yolo2_amd import engine as E
        self.E = E
        rng = np.random.default_rng(11)
        rows, total, flat = [], 0, []
        for (h, w) in ((5, 7), (8, 6)):                                   # the pool of two tiny images
            pitch = 16 * ((3 * w + 15) // 16)
            rows.append((total, h, w, pitch, 0))
            total += h * pitch
        self.pool = _cuda(rng.integers(0, 256, total, dtype=np.uint8), torch.uint8)
        self.table = _cuda(np.array(rows, np.int64), torch.int64)
        self.index = _cuda(np.array([1, 0], np.int32), torch.int32)
        self.labels = _cuda(np.array([7, 9], np.int32), torch.int32)
        self.params = _cuda(np.tile(np.array([1, 0, 0, 0, 1, 0, 1, 1, 1], np.float64), (n, 1)), torch.float64)
        self.predict = _cuda(rng.uniform(0, 1, (n, GRID, GRID, NCLS + 5 * B)), torch.float32)
        self.net = _cuda(rng.standard_normal((n, GRID, GRID, B, 5 + NCLS)), torch.float32)
        boxes = np.array([[[1, 1, 4, 3, 0], [2, 2, 6, 5, 1]], [[1, 2, 5, 8, 2], [0, 0, 0, 0, 0]]], np.float64)
        self.boxes = _cuda(boxes, torch.float64)
        self.counts = _cuda(np.array([2, 1], np.int32), torch.int32)
        self.difficult = _cuda(np.array([[0, 1], [0, 0]], np.uint8), torch.uint8)
        self.rows = E.detect_grid_batch(self.predict, self.table, self.index, NCLS, B, max_out=MAX_OUT)
        self.class_rows = E.detect_anchor_classes_batch_darknet(self.net, ANCHORS, self.table, self.index,
                                                                max_per_class=PER_CLASS, net_size=NET_SIZE)
        self.class_index = self.index.repeat_interleave(NCLS).contiguous()

    def call(self, name, out=None, **changed):
        """wrapper `name` on the kit's inputs, any of them replaced through `changed`; `out` as the wrapper takes it"""
        E = self.E
        a = dict(pool=self.pool, table=self.table, index=self.index, params=self.params, labels=None, labels_out=None,
                 anchors=ANCHORS, net_size=NET_SIZE, n=n)
        a.update(changed)
        if name == "detect_grid_batch":
            return E.detect_grid_batch(self.predict, a["table"], a["index"], NCLS, B, max_out=MAX_OUT, out=out)
        if name in ("letterbox_batch", "letterbox_darknet_batch"):
            return getattr(E, name)(a["pool"], a["table"], a["index"], a["n"], CANVAS, out=out)
        if name == "warp_batch":
            return E.warp_batch(a["pool"], a["table"], a["index"], a["n"], CANVAS, a["params"], labels=a["labels"], out=out,
                                labels_out=a["labels_out"])
        if name == "detect_anchor_batch":
            return E.detect_anchor_batch(self.net, a["anchors"], a["table"], a["index"], max_out=MAX_OUT, out=out,
                                         net_size=a["net_size"])
        if name in ANCHOR_DETECTS:
            return getattr(E, name)(self.net, a["anchors"], a["table"], a["index"], max_per_class=PER_CLASS, out=out,
                                    net_size=a["net_size"])
        if name == "voc_match_batch":
            det, score, count = self.rows
            return E.voc_match_batch(det, score, count, self.boxes, self.counts, self.difficult, a["index"], out=out)
        assert name == "voc_match_batch_f"
        det, score, count = self.class_rows
        index = self.class_index if a["index"] is self.index else a["index"]
        return E.voc_match_batch_f(det.view(n * NCLS, PER_CLASS, 6), score.view(n * NCLS, PER_CLASS), count.view(-1),
                                   self.boxes, self.counts, self.difficult, index, out=out)


@pytest.fixture(scope="module")
def kit():
    return Kit()


def _tensors(result):
    return result if isinstance(result, tuple) else (result,)


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and torch.equal(g.reshape(-1), w.reshape(-1))


# ---------------------------------------------------------------- 1. `out`: identity, and views of the right count
@pytest.mark.parametrize("name", NINE)
def test_out_tensors_come_back_by_identity_and_may_be_views(kit, name):
    want = _tensors(kit.call(name))
    for flat in (False, True):                                            # the documented shape, then a flat view of it
        mine = tuple(torch.empty(w.shape, dtype=w.dtype, device="cuda") for w in want)
        if flat:
            mine = tuple(m.view(-1) for m in mine)
        got = _tensors(kit.call(name, out=mine if len(mine) > 1 else mine[0]))
        assert all(g is m for g, m in zip(got, mine)), (name, flat)
        _same(got, want)
    wrong = tuple(torch.empty(w.numel() + 1, dtype=w.dtype, device="cuda") for w in want)
    with pytest.raises(AssertionError):
        kit.call(name, out=wrong if len(wrong) > 1 else wrong[0])


def test_warp_batch_returns_the_callers_labels_out(kit):
    want_out, want_labels = kit.call("warp_batch", labels=kit.labels)
    assert want_labels.cpu().tolist() == [9, 7]                           # labels[index]
    out = torch.empty(n * CANVAS * CANVAS * 3, dtype=torch.uint8, device="cuda")
    labels_out = torch.empty(n + 3, dtype=torch.int32, device="cuda")     # at least n
    got = kit.call("warp_batch", labels=kit.labels, out=out, labels_out=labels_out)
    assert got[0] is out and got[1] is labels_out
    _same((out, labels_out[:n]), (want_out, want_labels))
    with pytest.raises(AssertionError):
        kit.call("warp_batch", labels_out=labels_out)                     # labels_out without labels
    with pytest.raises(AssertionError):
        kit.call("warp_batch", labels=kit.labels, labels_out=labels_out[:1])


def test_score_views_takes_exact_shapes_only(kit):
    E = kit.E
    logits = _cuda(np.random.default_rng(3).standard_normal((4, 5)), torch.float32)       # 2 images, 2 views
    labels = _cuda(np.array([1, 4], np.int32), torch.int32)
    want = E.score_views(logits, labels, views=2, k=3, want_prob=True)
    own = dict(top_idx=torch.empty((2, 3), dtype=torch.int32, device="cuda"),
               top_val=torch.empty((2, 3), dtype=torch.float32, device="cuda"),
               rank=torch.empty((2,), dtype=torch.int32, device="cuda"),
               hits=torch.zeros(4, dtype=torch.int32, device="cuda"),
               prob=torch.empty((2, 5), dtype=torch.float32, device="cuda"))
    top_idx, top_val, rank, hits, prob = E.score_views(logits, labels, views=2, k=3, **own)
    assert top_idx is own["top_idx"] and top_val is own["top_val"] and rank is own["rank"]
    assert hits is own["hits"] and prob is own["prob"]
    _same((top_idx, top_val, rank, hits, prob), want)
    for key, t in own.items():                                            # the right count in another shape: refused
        other = t.reshape(-1, 1) if t.dim() == 1 else t.reshape(-1)
        with pytest.raises(AssertionError):
            E.score_views(logits, labels, views=2, k=3, **dict(own, **{key: other}))
    with pytest.raises(AssertionError):
        E.score_views(logits, None, views=2, k=3, rank=own["rank"])       # rank needs labels
    with pytest.raises(ValueError) as e:
        E.score_views(logits, labels, views=3)
    assert str(e.value) == "4 rows of logits are not a positive multiple of views = 3"


# ---------------------------------------------------------------- 2. malformed tensors: AssertionError, no launch
def _malformed(t, kind):
    if kind == "dtype":
        return t.to(torch.int16)
    if kind == "host":
        return t.cpu()
    wide = torch.stack((t, t), dim=-1)                                    # [..., 2]: every other element of it
    return wide[..., 0]


@pytest.mark.parametrize("kind", ("dtype", "host", "strided"))
def test_malformed_tensors_are_assertion_errors(kit, kind):
    assert not _malformed(kit.table, "strided").is_contiguous() and _malformed(kit.table, "strided").shape[-1] == 5
    for name in NINE:
        with pytest.raises(AssertionError):
            kit.call(name, index=_malformed(kit.class_index if name == "voc_match_batch_f" else kit.index, kind))
        if "voc_match" in name:
            continue                                                      # the matchers have no table
        with pytest.raises(AssertionError):
            kit.call(name, table=_malformed(kit.table, kind))
    for name in ("letterbox_batch", "warp_batch", "letterbox_darknet_batch"):
        with pytest.raises(AssertionError):
            kit.call(name, pool=_malformed(kit.pool, kind))
    with pytest.raises(AssertionError):
        kit.call("warp_batch", params=_malformed(kit.params, kind))
    with pytest.raises(AssertionError):
        kit.call("warp_batch", labels=_malformed(kit.labels, kind))
    for name in ANCHOR_DETECTS:                                           # a tensor of anchors is taken as it is
        with pytest.raises(AssertionError):
            kit.call(name, anchors=_malformed(_cuda(np.array(ANCHORS), torch.float32), kind))


def test_too_few_entries_are_assertion_errors(kit):
    for name in NINE:
        with pytest.raises(AssertionError):
            kit.call(name, index=kit.index[:1])                           # an index shorter than n
    for name in NINE:
        if "voc_match" not in name:
            with pytest.raises(AssertionError):
                kit.call(name, index=None, table=kit.table[:1])           # no index: the table bounds n
    E = kit.E
    det, score, count = kit.rows
    for match in (E.voc_match_batch, E.voc_match_batch_f):                # no index, no table: `boxes` bounds n
        with pytest.raises(AssertionError):
            match(det, score, count, kit.boxes[:1], kit.counts[:1], kit.difficult[:1])
        assert match(det, score, count, kit.boxes, kit.counts, kit.difficult).shape == (n, MAX_OUT)
    with pytest.raises(AssertionError):
        kit.call("warp_batch", params=kit.params[:1])                     # fewer than 9 n parameters


# ---------------------------------------------------------------- 3. the ValueError texts
def test_net_size_value_errors_keep_their_texts(kit):
    for name in ANCHOR_DETECTS:
        with pytest.raises(ValueError) as e:
            kit.call(name, net_size=96)
        assert str(e.value) == "net_size 96 is not the positive multiple of 32 that S = 2 makes (64)"
    with pytest.raises(ValueError) as e:
        kit.call("detect_anchor_classes_batch_darknet", net_size=None)
    assert str(e.value) == "detect_anchor_classes_batch_darknet needs net_size: Darknet's protocol is letterboxed"
    with pytest.raises(ValueError) as e:
        kit.E.yolov2_loss_boxes(kit.net, torch.zeros((n, 1, 5), device="cuda"),
                                torch.zeros(n, dtype=torch.int32, device="cuda"), ANCHORS, NET_SIZE, scales={"iou": 1.0})
    assert str(e.value) == "unknown loss scales ['iou']"


# ---------------------------------------------------------------- 4. anchors: list, array, device tensor
@pytest.mark.parametrize("name", ANCHOR_DETECTS)
def test_anchors_as_list_array_and_device_tensor_agree(kit, name):
    want = kit.call(name, anchors=[list(a) for a in ANCHORS])
    _same(kit.call(name, anchors=np.array(ANCHORS, np.float64)), want)
    _same(kit.call(name, anchors=_cuda(np.array(ANCHORS), torch.float32)), want)
    _same(kit.call(name, anchors=_cuda(np.array(ANCHORS), torch.float32).reshape(-1)), want)    # 2 B values, any shape
    for wrong in (ANCHORS + ((1.0, 1.0),), _cuda(np.ones((B + 1, 2)), torch.float32), ANCHORS[:1]):
        with pytest.raises(AssertionError):
            kit.call(name, anchors=wrong)


def test_the_loss_and_decode_calls_upload_their_anchors(kit):
    E = kit.E
    truth = torch.zeros((n, 1, 5), device="cuda")
    ntruth = torch.zeros(n, dtype=torch.int32, device="cuda")
    labels = torch.zeros((n, GRID, GRID, 5 + NCLS), device="cuda")
    for anchors in (ANCHORS, np.array(ANCHORS), torch.tensor(ANCHORS)):               # a HOST tensor is read by numpy
        _same(E.decode_anchors(kit.net, anchors), E.decode_anchors(kit.net, [list(a) for a in ANCHORS]))
        _same(E.yolov2_loss(kit.net, labels, anchors, NET_SIZE), E.yolov2_loss(kit.net, labels, ANCHORS, NET_SIZE))
        _same(E.yolov2_loss_boxes(kit.net, truth, ntruth, anchors, NET_SIZE),
              E.yolov2_loss_boxes(kit.net, truth, ntruth, ANCHORS, NET_SIZE))
    with pytest.raises(AssertionError):                                   # this one checks the shape, [B, 2]
        E.yolov2_loss_boxes(kit.net, truth, ntruth, np.array(ANCHORS).reshape(-1), NET_SIZE)
    with pytest.raises(TypeError):                                        # numpy does not read device memory
        E.decode_anchors(kit.net, _cuda(np.array(ANCHORS), torch.float32))


# ---------------------------------------------------------------- 5. the library's own messages, one per shared check
def _last_error():
    from tensorflow_yolo2_amd import _lib as L
    return L.load().y2_last_error().decode()


def test_shared_host_checks_keep_their_messages(kit):
    """every case fails in the entry's host check: nothing is launched (the buffer the pointers name stays as it is)"""
    from tensorflow_yolo2_amd import _lib as L
    E, lib = kit.E, L.load()
    buf = torch.full((1 << 12,), 5, dtype=torch.int32, device="cuda")
    before = buf.clone()
    p = C.c_void_p(buf.data_ptr())
    for entry in ANCHOR_ENTRIES:
        per_class, letterboxed = "classes" in entry, entry.endswith(("_lb", "_dk"))
        rows_name = "max_per_class" if per_class else "max_out"

        def call(n_=n, S_=GRID, B_=B, C_=NCLS, rows=2, net_size=NET_SIZE, net=p):
            size = (net_size,) if letterboxed else ()
            return getattr(lib, entry)(net, p, p, None, n_, S_, B_, C_, 0.1, 0.5, rows, *size, p, p, p, None)
        cases = [(dict(net=None), "null pointer"),
                 (dict(n_=0), "n = 0 outside 1..65535" if per_class else "n = 0"),
                 (dict(rows=0), "%s = 0" % rows_name),
                 (dict(B_=17), "S = 2, B = 17 (at most 16), num_class = 3"),
                 (dict(C_=0), "S = 2, B = 2 (at most 16), num_class = 0"),
                 (dict(S_=21, B_=5, net_size=672),
                  "S * S * B = 2205 candidates beyond Y2_DETECT_ANCHOR_MAX_CANDIDATES = 2048"),
                 # the order of the checks: an input that breaks two rules reports the earlier one
                 (dict(n_=0, rows=0, B_=17), "n = 0 outside 1..65535" if per_class else "n = 0"),
                 (dict(rows=0, B_=17, net_size=96), "%s = 0" % rows_name),
                 (dict(B_=17, net_size=96), "S = 2, B = 17 (at most 16), num_class = 3")]
        if per_class:
            cases.append((dict(n_=65536), "n = 65536 outside 1..65535"))
        if letterboxed:
            cases.append((dict(net_size=96),
                          "net_size = 96 is not the positive multiple of 32 that S = 2 makes (32 S = 64)"))
            cases.append((dict(net_size=0), "net_size = 0 is not the positive multiple of 32 that S = 2 makes (32 S = 64)"))
        for changed, text in cases:
            assert call(**changed) == -1, (entry, changed)
            assert _last_error() == "%s: %s" % (entry, text), (entry, changed)
    for entry in ("y2_voc_match_batch", "y2_voc_match_batch_f"):
        def match(det=p, n_=n, max_obj=2, max_out=MAX_OUT):
            return getattr(lib, entry)(det, p, p, p, p, p, None, n_, max_obj, max_out, 0.5, p, None)
        for changed, text in ((dict(det=None), "null pointer"), (dict(n_=0), "n = 0"), (dict(max_out=0), "max_out = 0"),
                              (dict(max_obj=0), "max_obj = 0 outside 1..Y2_MATCH_MAX_OBJECTS = 1024"),
                              (dict(max_obj=1025), "max_obj = 1025 outside 1..Y2_MATCH_MAX_OBJECTS = 1024"),
                              (dict(n_=0, max_out=0, max_obj=0), "n = 0")):
            assert match(**changed) == -1, (entry, changed)
            assert _last_error() == "%s: %s" % (entry, text), (entry, changed)
    # through the wrappers, with legal tensors whose sizes the library refuses
    wide = torch.zeros((n, GRID, GRID, 17, 5 + NCLS), device="cuda")
    many = torch.zeros((1, 12, 12, 16, 6), device="cuda")                # 2304 candidates
    for name, entry in (("detect_anchor_batch", "y2_detect_anchor_batch_lb"),
                        ("detect_anchor_classes_batch", "y2_detect_anchor_classes_batch_lb"),
                        ("detect_anchor_classes_batch_darknet", "y2_detect_anchor_classes_batch_dk")):
        with pytest.raises(L.Y2Error):
            getattr(E, name)(wide, np.ones((17, 2)), kit.table, kit.index, net_size=NET_SIZE)
        assert _last_error() == entry + ": S = 2, B = 17 (at most 16), num_class = 3"
        with pytest.raises(L.Y2Error):
            getattr(E, name)(many, np.ones((16, 2)), kit.table, kit.index, net_size=384)
        assert _last_error() == entry + ": S * S * B = 2304 candidates beyond Y2_DETECT_ANCHOR_MAX_CANDIDATES = 2048"
    for name, entry in (("detect_anchor_batch", "y2_detect_anchor_batch"),
                        ("detect_anchor_classes_batch", "y2_detect_anchor_classes_batch")):
        with pytest.raises(L.Y2Error):
            getattr(E, name)(wide, np.ones((17, 2)), kit.table, kit.index)
        assert _last_error() == entry + ": S = 2, B = 17 (at most 16), num_class = 3"
    det, score, count = kit.rows
    tall = torch.zeros((n, 1025, 5), dtype=torch.float64, device="cuda")
    hard = torch.zeros((n, 1025), dtype=torch.uint8, device="cuda")
    for name in ("voc_match_batch", "voc_match_batch_f"):
        with pytest.raises(L.Y2Error):
            getattr(E, name)(det, score, count, tall, kit.counts, hard, kit.index)
        assert _last_error() == "y2_%s: max_obj = 1025 outside 1..Y2_MATCH_MAX_OBJECTS = 1024" % name
    torch.cuda.synchronize()
    assert torch.equal(buf, before)


# ---------------------------------------------------------------- 6. the optimizers: what their shared base holds
def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32).copy()


# the solver tests' SPEC steps on gradients that are written into the buffer; its widths 96 and 125 have no weight-gradient
# launch, so the tests that run a backward pass take the same three layers at widths that have one
BACKWARD_SPEC = [(3, 3, 32, 1), (3, 32, 64, 0), (1, 64, 30, 0)]


def _net(dtype, training=True, spec=SPEC):
    from tensorflow_yolo2_amd import engine as E
    net = E.Network(spec, BATCH, SIZE, SIZE, dtype=dtype, training=training)
    net.init_params(5)
    return net


def _optimizer(kind, net, guard, fused_pack):
    from tensorflow_yolo2_amd import engine as E
    if kind == "adam":
        return E.AdamOptimizer(net, guard=guard, fused_pack=fused_pack)
    if kind == "momentum":
        return E.MomentumOptimizer(net, guard=guard, fused_pack=fused_pack)
    return E.DarknetSGD(net, S.Solver(burn_in=3, steps=(3,), scales=(0.5,)), guard=guard, fused_pack=fused_pack)


SLOTS = {"adam": ("m", "v"), "momentum": ("accum",), "sgd": ("accum",)}


@pytest.mark.parametrize("fused_pack", (True, False), ids=("packed", "flat"))
@pytest.mark.parametrize("guard", (True, False), ids=("guard", "plain"))
@pytest.mark.parametrize("kind", ("adam", "momentum", "sgd"))
def test_optimizer_state_round_trip(kind, guard, fused_pack):
    net = _net("f16" if guard else "f32")
    opt = _optimizer(kind, net, guard, fused_pack)
    assert opt.net is net and opt.guard is guard and opt.fused_pack is fused_pack and (opt.scaler is not None) == guard
    assert hasattr(opt, "t") == (kind != "momentum")
    rng = np.random.default_rng(2)
    for _ in range(2):
        net.grads.copy_(_cuda(rng.standard_normal(net.n_params) * 1e-2, torch.float32))
        opt.step(full_check=True)
    st = opt.export_state()
    assert set(st) == set(SLOTS[kind]) | ({"t"} if kind != "momentum" else set())
    if kind != "momentum":
        assert st["t"] == 2 and opt.t == 2 and type(st["t"]) is int
    for k in SLOTS[kind]:
        assert st[k].dtype == np.float32 and st[k].any()
        assert (st[k].view(np.uint32) == _bits(getattr(opt, k))).all()
    fresh = _optimizer(kind, _net("f16" if guard else "f32"), guard, fused_pack)
    if kind != "momentum":
        st["t"] = 7                                                       # any step, not only the one just exported
    fresh.load_state(st)
    for k in SLOTS[kind]:
        assert (_bits(getattr(fresh, k)) == st[k].view(np.uint32)).all()
    if kind != "momentum":
        assert fresh.t == 7
        if guard:
            assert fresh.scaler.ctrl.cpu().tolist()[:3] == [0, 7, 0] and fresh.scaler.state()[1] == 7
            assert fresh.export_state()["t"] == 7                         # the device counter, read back
            assert opt.scaler.state()[1] == 2


def test_darknet_sgd_refuses_an_inference_binding_before_any_launch():
    net = _net("f32", training=False)
    opt = _optimizer("sgd", net, False, True)
    before = _bits(net.params)
    with pytest.raises(ValueError) as e:
        opt.step()
    assert str(e.value) == "DarknetSGD steps a context bound for training"
    torch.cuda.synchronize()
    assert (_bits(net.params) == before).all() and not opt.accum.any()


@pytest.mark.parametrize("guard", (True, False), ids=("guard", "plain"))
@pytest.mark.parametrize("kind", ("adam", "momentum", "sgd"))
def test_backward_step_without_the_packed_step_is_backward_then_step(kind, guard):
    rng = np.random.default_rng(4)
    dtype = "f16" if guard else "f32"
    x = _cuda(rng.uniform(-1, 1, (BATCH, SIZE, SIZE, 3)), torch.float32)
    results = []
    for one_call in (True, False):
        net = _net(dtype, spec=BACKWARD_SPEC)
        opt = _optimizer(kind, net, guard, False)
        out = net.forward(x, True, True)
        dout = _cuda(np.random.default_rng(6).standard_normal(tuple(out.shape)) * 1e-3, torch.float32)
        if one_call:
            opt.backward_step(dout, grad_mult=0.5)
        else:
            net.backward(dout)
            opt.step(grad_mult=0.5)
        torch.cuda.synchronize()
        ctrl = opt.scaler.ctrl.cpu().tolist() if guard else None
        results.append([_bits(net.params), _bits(net.grads)] + [_bits(getattr(opt, k)) for k in SLOTS[kind]] + [ctrl])
    assert (results[0][0] != _bits(_net(dtype, spec=BACKWARD_SPEC).params)).any()             # the step moved the parameters
    for a, b in zip(*results):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b
