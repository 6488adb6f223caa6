"""The wide head on the GPU (csrc/wide_head.hip): y2_wide_head_forward against numpy float64 on the f16-rounded operands,
against the linear last layer of an engine.Network stack, its packed image, its argument errors, and a detector built
from tests/golden/cfg/chain-wide.cfg through load, save, forward and detect_batch.

Kernel parity.  With x and W rounded to f16 the products are exact in fp32, so only the accumulation order differs from the
reference: per element |got - ref| <= 2 K 2^-24 sum_k |x_k w_k| + 1e-30, the fp32 recursive-summation bound of any order
doubled for the MFMA's internal adds (tests/_wide_head_cases.py says why the bias stays within that sum's order)."""
import ctypes

import numpy as np
import pytest

import _wide_head_cases as K
from tensorflow_yolo2_amd.utils import detect_batch as DB, word_tree as W

gpu = pytest.mark.gpu
MARGIN = 1e-5


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _packed(lib, Wd, Kdim, Cout):
    return K.packed_image(lib, Wd, Kdim, Cout)


@gpu
@pytest.mark.parametrize("M,Kdim,Cout", K.GEMM_SHAPES)
def test_forward_matches_float64_on_the_f16_operands(M, Kdim, Cout):
    K.check_forward_on_the_device(*K.gemm_operands(M, Kdim, Cout))


@gpu
def test_forward_equals_the_linear_last_layer_of_a_stack():
    """(147, 128, 225): the same filters as the one-layer f16 stack (1, 128, 225), linear, its inference batch norm the
    identity the Darknet importer writes -- the project's per-layer convention, rel_to_max <= 1e-3"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import darknet_weights as dkw
    M, Kdim, Cout = 147, 128, 225
    x, Wt, b = K.gemm_operands(M, Kdim, Cout)
    net = E.Network([(1, Kdim, Cout, 0)], 3, 7, 7, dtype="f16", training=False)
    net.set_layer_options(slopes=[1.0], bn_eps=1e-6)
    file_form = {"biases": b, "weights": np.ascontiguousarray(Wt.T).reshape(Cout, Kdim, 1, 1)}
    net.load_params([dkw.to_layer_params(file_form, 1, 1e-6)])
    want = net.forward(dev(x.reshape(3, 7, 7, Kdim)), False, False).cpu().numpy().reshape(M, Cout)
    wide = E.WideHead(Kdim, Cout)
    wide.load(Wt, b)
    got = wide.forward(dev(x)).cpu().numpy()
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("wide head against the stack's last layer: rel_to_max %.3e" % rel)
    assert rel <= 1e-3, rel


@gpu
def test_pack_pads_with_zeros_and_export_returns_what_load_was_given():
    import torch
    from tensorflow_yolo2_amd import _lib, engine as E
    lib = _lib.load()
    Kdim, Cout = 96, 225                                                  # K rounds up to 128, Cout to 256
    _x, Wt, b = K.gemm_operands(7, Kdim, Cout)
    packed = _packed(lib, dev(Wt), Kdim, Cout)
    torch.cuda.synchronize()
    image = packed.cpu().numpy().view(np.float16).reshape(256, 128)
    assert np.array_equal(image[:Cout, :Kdim].view(np.uint16), np.ascontiguousarray(Wt.T).astype(np.float16).view(np.uint16))
    assert not image[Cout:].view(np.uint16).any() and not image[:, Kdim:].view(np.uint16).any()   # +0.0 halves
    wide = E.WideHead(Kdim, Cout)
    assert not wide.packed.cpu().numpy().any()                            # a fresh operator: zero filters, packed
    wide.load(Wt.reshape(1, 1, Kdim, Cout), b)
    back = wide.export()
    assert back["W"].shape == (1, 1, Kdim, Cout) and back["W"].dtype == np.float32
    assert np.array_equal(back["W"].view(np.uint32).ravel(), Wt.view(np.uint32).ravel())
    assert np.array_equal(back["b"].view(np.uint32), b.view(np.uint32))
    assert np.array_equal(wide.packed.cpu().numpy(), packed.cpu().numpy())
    with pytest.raises(ValueError, match="do not fit"):
        wide.load(Wt[:, :-1], b)
    with pytest.raises(ValueError, match="multiple of 32"):
        E.WideHead(100, 10)


@gpu
def test_wide_head_entries_reject_bad_arguments():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    M, Kdim, Cout = 5, 64, 200
    x, Wt, b = K.gemm_operands(M, Kdim, Cout)
    xd, Wd, bd = dev(x), dev(Wt), dev(b)
    nbytes = lib.y2_wide_head_packed_bytes(Kdim, Cout)
    packed = torch.full((nbytes + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full((M * Cout,), 7.0, device="cuda")
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    forward = (("x", p(xd)), ("packed", p(packed)), ("bias", p(bd)), ("M", M), ("K", Kdim), ("Cout", Cout), ("out", p(out)),
               ("stream", None))
    pack = (("W", p(Wd)), ("K", Kdim), ("Cout", Cout), ("packed", p(packed)), ("bytes", nbytes), ("stream", None))
    shared = ((dict(K=0), b"K = 0"), (dict(K=48), b"multiple of 32"), (dict(K=4128), b"at most 4096"),
              (dict(Cout=0), b"Cout = 0"), (dict(Cout=65536 * 16 + 1), b"Cout = 1048577"), (dict(packed=None), b"null"),
              (dict(packed=off(packed, 8)), b"16-byte aligned"))
    more = {"y2_wide_head_forward": ((dict(M=0), b"M = 0"), (dict(M=-3), b"at least 1"), (dict(x=None), b"null"),
                                     (dict(bias=None), b"null"), (dict(out=None), b"null"),
                                     (dict(x=off(xd, 4)), b"16-byte aligned")),
            "y2_wide_head_pack": ((dict(W=None), b"null"), (dict(bytes=nbytes - 1), b"packed_bytes"))}
    for name, table in (("y2_wide_head_forward", forward), ("y2_wide_head_pack", pack)):
        call = lambda **kw: getattr(lib, name)(*[kw.get(k, v) for k, v in table])
        for kw, word in shared + more[name]:
            assert call(**kw) == -1, (name, kw)                           # Y2_ERR_ARG
            err = lib.y2_last_error()
            assert name.encode() in err and word in err, (name, kw, err)
    for bad in ((0, 10), (48, 10), (4128, 10), (64, 0), (64, 65536 * 16 + 1)):
        assert lib.y2_wide_head_packed_bytes(*bad) == 0, bad
    assert lib.y2_wide_head_packed_bytes(4096, 65536 * 16) == 4096 * 65536 * 16 * 2
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (packed == 0xAB).all()                  # nothing was launched
    assert lib.y2_wide_head_pack(*[v for _k, v in pack]) == 0 and lib.y2_wide_head_forward(*[v for _k, v in forward]) == 0
    torch.cuda.synchronize()
    assert not (out == 7.0).any() and (packed[nbytes:] == 0xAB).all()


@gpu
def test_detector_from_the_wide_cfg_end_to_end(tmp_path):
    """chain-wide.cfg at 160 x 160 (S = 5), batch 2: a `.weights` round trip, the raw head against WideHead.forward of the
    head stack's own output, detect_batch against the host specification fed with the device's raw head, the refusals"""
    import torch
    from test_gpu_detect_anchor import SHAPES, _table
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    n, S, thresh, iou, max_out = 2, 5, 0.05, 0.45, 20
    cfg = K.write_wide_model_files(tmp_path)
    det = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16", seed=3, wide_head=True)
    assert det.wide is not None and (det.wide.K, det.wide.Cout) == (128, 2115) and det.cfg.map == "x.map"
    assert det.tree is not None and det.tree.n == 700 == det.num_class and det.B == 3 and det.tree_thresh == 0.4
    assert [len(net.spec) for net in det.networks()] == [6, 2] and det.head.spec[-1] == (3, 128, 128, 0)
    # load -> save: the bytes read
    src = K.random_weights_file(str(tmp_path / "wide.weights"), det.cfg.file_layers, seed=21)
    assert net_utils.load_darknet_weights(det, src) == 1234
    back = str(tmp_path / "back.weights")
    net_utils.save_darknet_weights(det, back, 1234)
    with open(src, "rb") as f, open(back, "rb") as g:
        data = f.read()
        assert data == g.read() and len(data) == 16 + 4 * det.cfg.floats
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8))
    table = torch.from_numpy(_table()).cuda()
    raw = torch.full((n, S, S, 3, 705), float("nan"), device="cuda")
    d, s, c = det.detect_batch(x, table, None, thresh, iou, max_out, grid_out=raw)
    torch.cuda.synchronize()
    # the raw head is the wide operator on the head stack's own output, bit for bit
    stack_out = det.head._out
    assert tuple(stack_out.shape) == (n, S, S, 128)
    again = det.wide.forward(stack_out, out=torch.empty(n * S * S * 2115, device="cuda"))
    assert np.array_equal(again.cpu().numpy().view(np.uint32), raw.cpu().numpy().view(np.uint32).ravel())
    head = raw.cpu().numpy().reshape(-1, 705)
    assert np.isfinite(head).all() and head[:, 5:].std() > 0.3
    # the host specification from the device's raw head: the tree walk, then the rows
    spec_head, top, _prob, m = W.word_tree_head(head, det.tree.tree, det.tree_thresh, return_margins=True)
    assert m["thresh"] >= MARGIN and m["group_gap"] >= MARGIN, m
    assert len(set(top.tolist())) > 10 and det.tree.tree.depth[top].max() >= 1
    boxes, scores = E.decode_anchors(dev(spec_head.astype(np.float32).reshape(n, S, S, 3, 705)), det.anchors)
    best, cls = E.class_argmax(scores)
    boxes, best, cls = (t.cpu().numpy() for t in (boxes, best, cls))
    assert np.array_equal(cls.ravel(), top)
    d, s, c = d.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()
    for k in range(n):
        want_det, want_score = DB.anchor_detect(boxes[k], best[k], cls[k], SHAPES[k][1], SHAPES[k][0], thresh, iou, max_out)
        cnt = len(want_det)
        assert c[k] == cnt and np.array_equal(d[k, :cnt], want_det), k
        assert np.array_equal(s[k, :cnt].view(np.uint32), want_score.view(np.uint32)), k
        assert (d[k, cnt:] == -1).all() and (s[k, cnt:] == 0).all()
    assert c.sum() > 0
    # detect() reads the same head
    _b, _best, cls2, _keep, _count = det.detect(x)
    assert np.array_equal(cls2.cpu().numpy().ravel(), top)
    # what a wide model refuses
    with pytest.raises(ValueError, match="detect_batch"):
        det.detect_classes_batch(x, table, None, thresh, iou, 8)
    for dtype in ("f32", "f16x2", "f16x2f"):
        with pytest.raises(ValueError, match="wide head"):
            yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype=dtype, wide_head=True)
    with pytest.raises(ValueError, match="map"):
        yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, dtype="f16")
    with pytest.raises(ValueError, match="map"):
        yolov2.YOLOv2DarknetTrainer.from_cfg(det.cfg, dtype="f16")       # a record that carries map, whoever parsed it
    with pytest.raises(ValueError, match="at most 2048"):
        yolov2.YOLOv2DarknetTrainer.from_cfg(K.write_wide_model_files(tmp_path, with_map=False), dtype="f16")
    with pytest.raises(ValueError, match="map"):
        yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16")   # the detector's default keyword, too
