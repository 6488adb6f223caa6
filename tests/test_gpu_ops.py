"""GPU parity tests (run with -m gpu on an MI355X): every call goes through the
C ABI of libyolo2_hip.so and is compared with the numpy oracle on the same seeded
inputs.  Tolerances: f32 mode 1e-3 relative (north_star; observed ~1e-6),
index work (object_mask, decode) bit-exact; f16/bf16 modes looser, stated per test."""
import numpy as np
import pytest
import torch

from oracle import nn_ref as R, loss_ref as L, optim_ref as O, data_ref as D
from _obs import gate

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def relerr(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def l2err(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# about twice the maxima observed on MI355X (gpurun_out/observed_errors.txt, round 2): f32 1.7e-6, f16 5.5e-4, bf16 3.9e-3
TOL = {"f32": 4e-6, "f16": 1.2e-3, "bf16": 8e-3}


def mesh(n):
    i = np.arange(n)
    return (i[:, None] + i[None, :]).astype(np.float32)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_conv2d_slim_kats(dtype):
    """reference KATs src/slim_dir/nets/resnet_v1_test.py:72-152 (small integers: exact in every dtype)."""
    from tensorflow_yolo2_amd import engine as E
    w = mesh(3).reshape(3, 3, 1, 1)
    y = E.conv2d(dev(mesh(4).reshape(1, 4, 4, 1)), dev(w), dtype=dtype).cpu().numpy()[0, :, :, 0]
    exp4 = np.array([[14, 28, 43, 26], [28, 48, 66, 37], [43, 66, 84, 46], [26, 37, 46, 22]], np.float32)
    np.testing.assert_array_equal(y, exp4)
    y = E.conv2d(dev(mesh(5).reshape(1, 5, 5, 1)), dev(w), dtype=dtype).cpu().numpy()[0, :, :, 0]
    exp5 = np.array([[14, 28, 43, 58, 34], [28, 48, 66, 84, 46], [43, 66, 84, 102, 55],
                     [58, 84, 102, 120, 64], [34, 46, 55, 64, 30]], np.float32)
    np.testing.assert_array_equal(y, exp5)
    np.testing.assert_array_equal(R.subsample(y[None, :, :, None], 2)[0, :, :, 0],
                                  [[14, 43, 34], [43, 84, 55], [34, 55, 30]])


CONV_CASES = [
    # N, H, W, Cin, Cout, k
    (2, 13, 13, 32, 64, 3),      # 64-byte K rows at f16, 256x64 tile
    (1, 9, 11, 64, 32, 3),       # 256x32 tile, ragged M
    (2, 8, 8, 128, 128, 3),      # 128x128 tile
    (1, 13, 13, 256, 128, 1),    # 1x1
    (3, 7, 5, 96, 160, 3),       # odd channel counts (padded internally), 64-byte K rows
    (1, 4, 4, 128, 30, 1),       # detector output layer shape
    (1, 26, 26, 64, 128, 3),
]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_vs_oracle(case, dtype):
    from tensorflow_yolo2_amd import engine as E
    n, h, w, ci, co, k = case
    rng = np.random.default_rng(hash(case) % 1000)
    x = rng.uniform(-1, 1, (n, h, w, ci)).astype(np.float32)
    wt = (rng.standard_normal((k, k, ci, co)) * 0.1).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, co).astype(np.float32)
    y = E.conv2d(dev(x), dev(wt), dev(b), dtype=dtype).cpu().numpy()
    ref = R.conv2d_same(x.astype(np.float64), wt.astype(np.float64)) + b
    gate("conv2d fwd %s" % dtype, relerr(y, ref), TOL[dtype])


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv2d_backward_vs_oracle(case, dtype):
    from tensorflow_yolo2_amd import engine as E
    n, h, w, ci, co, k = case
    rng = np.random.default_rng(hash(case) % 1000 + 1)
    x = rng.uniform(-1, 1, (n, h, w, ci)).astype(np.float32)
    wt = (rng.standard_normal((k, k, ci, co)) * 0.1).astype(np.float32)
    dy = rng.standard_normal((n, h, w, co)).astype(np.float32)
    dx, dw = E.conv2d_backward(dev(x), dev(wt), dev(dy), dtype=dtype)
    rdx, rdw = R.conv2d_same_backward(x.astype(np.float64), wt.astype(np.float64), dy.astype(np.float64))
    gate("conv2d dx %s" % dtype, relerr(dx.cpu().numpy(), rdx), TOL[dtype])
    gate("conv2d dw %s" % dtype, relerr(dw.cpu().numpy(), rdw), TOL[dtype])


def test_conv2d_edge_single_pixel_and_unit_batch():
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (1, 1, 1, 32)).astype(np.float32)
    wt = rng.standard_normal((3, 3, 32, 32)).astype(np.float32)
    y = E.conv2d(dev(x), dev(wt), dtype="f32").cpu().numpy()
    assert relerr(y, R.conv2d_same(x.astype(np.float64), wt.astype(np.float64))) < 1e-5


# ---------------------------------------------------------------------------
def _stack_case(first3):
    if first3:
        spec = [(3, 3, 32, 1), (3, 32, 64, 1), (1, 64, 32, 0), (3, 32, 128, 1), (3, 128, 30, 0)]
        shape = (3, 24, 20, 3)
    else:
        spec = [(3, 32, 64, 0), (1, 64, 128, 1), (3, 128, 64, 0)]
        shape = (2, 10, 14, 32)
    return spec, shape


def _rand_params(spec, rng):
    params = R.init_params(spec, seed=int(rng.integers(1 << 30)))
    for p in params:
        p["gamma"] = rng.uniform(0.5, 1.5, p["gamma"].shape).astype(np.float32)
        p["beta"] = rng.uniform(-0.3, 0.3, p["beta"].shape).astype(np.float32)
        p["b"] = rng.uniform(-0.2, 0.2, p["b"].shape).astype(np.float32)
        p["moving_mean"] = rng.uniform(-0.2, 0.2, p["b"].shape).astype(np.float32)
        p["moving_var"] = rng.uniform(0.5, 2.0, p["b"].shape).astype(np.float32)
    return params


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("first3", [True, False])
@pytest.mark.parametrize("training", [True, False])
def test_stack_forward(first3, training, dtype):
    from tensorflow_yolo2_amd import engine as E
    spec, shape = _stack_case(first3)
    rng = np.random.default_rng(11)
    params = _rand_params(spec, rng)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    net = E.Network(spec, shape[0], shape[1], shape[2], dtype=dtype, training=False)
    net.load_params(params)
    out = net.forward(dev(x), training, training, update_moving=True).cpu().numpy()
    ref, caches, movings = R.run_stack(x, params, spec, training, np.float64)
    tol = {"f32": 4e-6, "f16": 5e-3, "bf16": 3e-2}[dtype]   # observed 1.7e-6 / 2.5e-3 / 1.4e-2
    assert out.shape == ref.shape
    gate("stack forward vs unquantised oracle %s" % dtype, relerr(out, ref), tol)
    if training:   # UPDATE_OPS: moving <- 0.99 moving + 0.01 batch (biased variance)
        got = net.export_params()
        for l, mv in enumerate(movings):
            assert relerr(got[l]["moving_mean"], mv[0]) < max(tol, 1e-4)
            assert relerr(got[l]["moving_var"], mv[1]) < max(tol, 1e-4)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("first3", [True, False])
def test_stack_backward(first3, dtype):
    """Batch statistics; with the 3-channel first layer also the moving ones (forward(x, False, False) on the training
    binding): its linear-form backward then builds the Gram matrix of the input patches itself."""
    from tensorflow_yolo2_amd import engine as E
    spec, shape = _stack_case(first3)
    rng = np.random.default_rng(12)
    params = _rand_params(spec, rng)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    net = E.Network(spec, shape[0], shape[1], shape[2], dtype=dtype, training=True)
    net.load_params(params)
    for batch_bn in ((True, False) if first3 else (True,)):
        _stack_backward_case(net, x, params, spec, first3, dtype, batch_bn, rng)


def _stack_backward_case(net, x, params, spec, first3, dtype, batch_bn, rng):
    mode = "" if batch_bn else " moving statistics"
    out = net.forward(dev(x), batch_bn, batch_bn)
    # f32 mode is checked against the exact reference semantics.  The half modes are
    # the exact gradient of a function that differs from the f32 one at max-pool /
    # leaky decisions (activations are STORED in half precision), so they are checked
    # against the oracle with the same storage points quantised (oracle quantizer()).
    q = R.quantizer(dtype)
    # The pooled 3-channel first layer of the half modes takes its batch moments from the Gram matrix of the input
    # patches (moments of the UN-rounded conv output, fp32 MFMA sums).  The oracle is not taught that form: it is handed
    # the moments the device normalised with as INPUTS of layer 0 (y2_debug_read selector 3), and those moments are
    # gated on their own against float64 in test_first_layer_statistics_from_the_gram_matrix (1e-4).  With the same
    # moments on both sides the stored half-precision activations agree again to the rounding of the arithmetic between
    # the storage points (the round-4 gates bf16 8e-3 / f16 2e-3 are back at 1e-6 / 1e-3).
    if q is None:
        ref, caches, _ = R.run_stack(x, params, spec, batch_bn, np.float64)
        gate("stack forward vs oracle f32 first3=%d%s" % (first3, mode), l2err(out.cpu().numpy(), ref), 4e-6)   # observed 1.5e-6
    else:
        # The oracle runs layer by layer on the device's stored inputs and the storage-rounding flips are gated as flips
        # (few, a few ulps: tests/_shapes.py teacher_forced_stack); the fp32 network output, given the device's input of
        # the last layer, is then held to fp32 round-off in BOTH half types (round 3's gates were 1e-3 / 1e-6 on the
        # free-running stack, round 4's 2e-3 / 8e-3)
        from _shapes import teacher_forced_stack
        first_stats = None
        if first3 and batch_bn:
            st = net.layer_statistics(0)
            first_stats = (st["mean"], st["var"])
        ref, caches, report = teacher_forced_stack(net, x, params, spec, dtype, first_stats, is_training=batch_bn)
        print("stored activations that differ from the quantised oracle (layer, count, of, worst ulps):", report)
        gate("stack forward vs quantised oracle %s first3=%d%s" % (dtype, first3, mode), l2err(out.cpu().numpy(), ref), 5e-5)
    dout = rng.standard_normal(ref.shape).astype(np.float32)
    net.backward(dev(dout))
    _, rgrads = R.run_stack_backward(params, caches, dout.astype(np.float64), np.float64, quant=q,
                                     grad_scale=net.grad_scale)
    grads = net.export_grads()
    tol = {"f32": 5e-6, "f16": 4e-3, "bf16": 1e-2}[dtype]    # observed 1.7e-6 / 1.9e-3 / 4.3e-3
    for l in range(len(spec)):
        for k in ("W", "gamma", "beta") if batch_bn else ("W", "gamma", "beta", "b"):
            gate("stack backward %s first3=%d%s" % (dtype, first3, mode), l2err(grads[l][k], rgrads[l][k]), tol)
        if batch_bn:   # conv bias gradient is mathematically zero under batch-stat BN: absolute check
            scale = np.abs(rgrads[l]["gamma"]).max() + np.abs(rgrads[l]["beta"]).max()
            assert np.abs(grads[l]["b"]).max() < 1e-2 * scale + 1e-3


def test_stack_backward_mixed_bn_modes():
    """core in inference-BN mode, head with batch statistics (pascal_detect_darknet.py:41-42 pattern)."""
    from tensorflow_yolo2_amd import engine as E
    spec, shape = _stack_case(False)
    rng = np.random.default_rng(13)
    params = _rand_params(spec, rng)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    net = E.Network(spec, shape[0], shape[1], shape[2], dtype="f32", training=False, core_layers=2)
    net.load_params(params)
    out = net.forward(dev(x), False, True).cpu().numpy()
    h, _, _ = R.run_stack(x, params[:2], spec[:2], False, np.float64)
    ref, _, _ = R.run_stack(h, params[2:], spec[2:], True, np.float64)
    assert relerr(out, ref) < 2e-5


# ---------------------------------------------------------------------------
def make_labels(rng, n, S, image_size, num_class=20):
    labels = np.zeros((n, S, S, 5 + num_class), np.float32)
    for i in range(n):
        objs = []
        for _ in range(rng.integers(1, 4)):
            x1, y1 = rng.uniform(1, image_size * 0.7, 2)
            bw, bh = rng.uniform(image_size * 0.05, image_size * 0.3, 2)
            objs.append((x1, y1, x1 + bw, y1 + bh, int(rng.integers(0, num_class))))
        labels[i] = D.encode_boxes(objs, image_size, image_size, image_size, S, num_class)
    return labels


@pytest.mark.parametrize("S,image_size,n", [(7, 224, 24), (13, 416, 64), (7, 224, 1), (3, 96, 5)])
def test_yolo_loss_vs_oracle(S, image_size, n):
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(S * 100 + n)
    B, C = 2, 20
    net = rng.uniform(-0.5, 1.2, (n, S, S, C + 5 * B)).astype(np.float32)
    labels = make_labels(rng, n, S, image_size)
    off = L.yolo_grid_offset(S, B)
    loss, ious, mask, dnet = E.yolo_loss(dev(net), dev(labels), C, n, image_size, S, B)
    # op-by-op float32 evaluation of the reference graph: ious / mask bit-identical
    t32, i32, m32, p32 = L.get_loss(net, labels, C, n, image_size, S, B, off, np.float32)
    np.testing.assert_array_equal(mask.cpu().numpy(), m32)
    np.testing.assert_array_equal(ious.cpu().numpy(), i32)
    t64, i64, m64, p64 = L.get_loss(net, labels, C, n, image_size, S, B, off, np.float64)
    lo = loss.cpu().numpy()
    for j, k in enumerate(("class_loss", "object_loss", "noobject_loss", "coord_loss")):
        assert abs(lo[j] - p64[k]) <= 1e-5 * max(abs(p64[k]), 1e-3), (k, lo[j], p64[k])
    assert abs(lo[4] - t64) <= 1e-5 * abs(t64)
    d64 = L.get_loss_backward(net, labels, C, n, image_size, S, B, off, np.float64)
    assert relerr(dnet.cpu().numpy(), d64) < 1e-5
    assert m32.sum() >= n and (i32 > 0.01).sum() > 0


def test_yolo_loss_empty_labels():
    from tensorflow_yolo2_amd import engine as E
    n, S, B, C = 2, 7, 2, 20
    rng = np.random.default_rng(0)
    net = rng.uniform(-0.5, 1.2, (n, S, S, C + 5 * B)).astype(np.float32)
    labels = np.zeros((n, S, S, 25), np.float32)
    loss, ious, mask, dnet = E.yolo_loss(dev(net), dev(labels), C, n, 224, S, B)
    t, i, m, p = L.get_loss(net, labels, C, n, 224, S, B, L.yolo_grid_offset(S, B), np.float32)
    assert mask.sum().item() == 0
    np.testing.assert_array_equal(ious.cpu().numpy(), i)
    assert abs(loss[4].item() - t) < 1e-5 * t


def test_get_iou_vs_oracle():
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(4)
    b1 = rng.uniform(0, 1, (5, 7, 7, 2, 4)).astype(np.float32)
    b2 = rng.uniform(0, 1, (5, 7, 7, 2, 4)).astype(np.float32)
    b2[0, 0, 0] = b1[0, 0, 0]            # identical boxes -> IoU 1
    b2[0, 0, 1, :, 2:] = 0.0             # degenerate boxes
    out = E.get_iou(dev(b1), dev(b2)).cpu().numpy()
    np.testing.assert_array_equal(out, L.get_iou(b1, b2))
    assert out[0, 0, 0, 0] == 1.0 or abs(out[0, 0, 0, 0] - 1) < 1e-6


def test_decode_vs_oracle():
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(5)
    for S, (im_w, im_h) in ((7, (353, 500)), (13, (352, 240))):
        p = rng.uniform(-0.2, 1.0, (S, S, 30)).astype(np.float32)
        got = E.decode_detections(dev(p), S, 2, 20, im_w, im_h)
        exp = L.decode_detections(p, im_w, im_h, 20, S, 2)
        assert len(exp) > 5
        assert [g[:5] + g[6:] for g in got] == [e[:5] + e[6:] for e in exp]
        np.testing.assert_array_equal([g[5] for g in got], [np.float32(e[5]) for e in exp])


def test_softmax_ce_vs_oracle():
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(6)
    logits = rng.standard_normal((16, 1000)).astype(np.float32) * 3
    labels = rng.integers(0, 1000, 16)
    loss, dl = E.softmax_cross_entropy(dev(logits), torch.as_tensor(labels).cuda())
    rl, rdl = R.sparse_softmax_cross_entropy_mean(logits.astype(np.float64), labels)
    assert abs(loss.item() - rl) < 1e-5 * rl
    assert relerr(dl.cpu().numpy(), rdl) < 1e-5


def test_optimizers_vs_oracle():
    from tensorflow_yolo2_amd import engine as E
    spec = [(3, 32, 32, 0)]
    net = E.Network(spec, 1, 4, 4, dtype="f32", training=True)
    rng = np.random.default_rng(7)
    p0 = rng.standard_normal(net.n_params).astype(np.float32)
    for opt_name in ("adam", "momentum"):
        net.params.copy_(dev(p0))
        opt = E.AdamOptimizer(net) if opt_name == "adam" else E.MomentumOptimizer(net)
        var = p0.copy(); m = np.zeros_like(p0); v = np.zeros_like(p0)
        for t in range(1, 4):
            g = rng.standard_normal(net.n_params).astype(np.float32)
            net.grads.copy_(dev(g))
            opt.step()
            if opt_name == "adam":
                var, m, v = O.adam_step(var, m, v, g, t, dtype=np.float64)
            else:
                var, m = O.momentum_step(var, m, g, dtype=np.float64)
        assert relerr(net.params.cpu().numpy(), var) < 1e-6


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("shape", [(2, 15, 13, 3), (1, 33, 47, 3), (2, 64, 96, 3)])
def test_first_layer_paths_odd_and_wide(shape, dtype):
    """The pooled first layer has a two-pass / recomputing / fused form for even sizes and falls back to
    conv1 + bn_act + apply + plain weight gradient for odd ones (SAME pooling pads bottom/right): both must
    match the oracle, forward and backward."""
    from tensorflow_yolo2_amd import engine as E
    spec = [(3, 3, 32, 1), (3, 32, 64, 1), (1, 64, 30, 0)]
    rng = np.random.default_rng(sum(shape))
    params = _rand_params(spec, rng)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    net = E.Network(spec, shape[0], shape[1], shape[2], dtype=dtype, training=True)
    net.load_params(params)
    out = net.forward(dev(x), True, True)
    q = R.quantizer(dtype)
    # even sizes: the linear-form path, whose batch moments come from the Gram matrix (un-rounded conv output); odd sizes:
    # conv1 + bn_act with the moments of the stored values.  Either way the oracle gets the moments the device normalised
    # layer 0 with as inputs (test_stack_backward above; the moments themselves are gated in test_gpu_kernel_policies.py)
    gram = shape[1] % 2 == 0 and shape[2] % 2 == 0
    if q is None:
        ref, caches, _ = R.run_stack(x, params, spec, True, np.float64)
        assert out.shape == ref.shape
        gate("first layer forward f32 gram=%d" % gram, l2err(out.cpu().numpy(), ref), 3e-6)      # 9.5e-7
    else:
        from _shapes import teacher_forced_stack
        st = net.layer_statistics(0)
        ref, caches, report = teacher_forced_stack(net, x, params, spec, dtype, (st["mean"], st["var"]))
        assert out.shape == ref.shape
        print("stored activations that differ from the quantised oracle (layer, count, of, worst ulps):", report)
        # (the last layer's conv output is stored in the half type too: each of ITS rounding flips is one ulp over
        #  sqrt(size) in l2 -- observed 1.3e-5 at 64 x 96)
        gate("first layer forward %s gram=%d" % (dtype, gram), l2err(out.cpu().numpy(), ref), 5e-5)
    dout = rng.standard_normal(ref.shape).astype(np.float32)
    net.backward(dev(dout))
    _, rgrads = R.run_stack_backward(params, caches, dout.astype(np.float64), np.float64, quant=q,
                                     grad_scale=net.grad_scale)
    grads = net.export_grads()
    # f16: dy and y are stored / staged in half precision (12 k pixels summed per filter element)
    tol = {"f32": 4e-6, "f16": 2.5e-2}[dtype]     # observed 1.2e-6 / 2.1e-2
    for l in range(len(spec)):
        for k in ("W", "gamma", "beta"):
            gate("first layer backward %s" % dtype, l2err(grads[l][k], rgrads[l][k]), tol)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_conv2d_random_shapes_forward_and_backward(dtype):
    """Seeded sweep over shapes that cross every kernel-policy boundary (rows <= 26 / 52 / 104 / wider, narrow and
    wide cout tiles, 16- and 32-row MFMA fragment packs, ring and windowed weight gradients, 1x1): forward, dx and
    dW of the single-op entry points against torch's CPU convolution."""
    import torch.nn.functional as F
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(2024)
    cases = [(2, 13, 13, 512, 1024, 3), (3, 26, 26, 256, 128, 3), (1, 52, 52, 128, 64, 3), (1, 104, 104, 64, 128, 3),
             (1, 104, 60, 128, 64, 3), (1, 40, 208, 32, 64, 3), (1, 30, 208, 64, 32, 3), (2, 19, 19, 160, 96, 3),
             (4, 7, 7, 1024, 512, 1), (2, 27, 25, 96, 160, 1), (8, 13, 13, 1024, 1024, 3), (1, 5, 37, 32, 32, 3)]
    for _ in range(6):
        cases.append((int(rng.integers(1, 4)), int(rng.integers(3, 60)), int(rng.integers(3, 120)),
                      int(rng.choice([32, 64, 96, 128, 256])), int(rng.choice([30, 32, 64, 128, 200, 256])),
                      int(rng.choice([1, 3]))))
    tol = {"f32": (5e-6, 5e-6), "f16": (8e-4, 8e-4)}[dtype]   # observed 1.9e-6 / 3.6e-4
    for (n, h, w, ci, co, k) in cases:
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        wt = (rng.standard_normal((k, k, ci, co)) / np.sqrt(k * k * ci)).astype(np.float32)
        dy = rng.standard_normal((n, h, w, co)).astype(np.float32)
        xt = torch.as_tensor(x).permute(0, 3, 1, 2).requires_grad_(True)
        wtt = torch.as_tensor(wt).permute(3, 2, 0, 1).requires_grad_(True)
        ref = F.conv2d(xt, wtt, padding=k // 2)
        ref.backward(torch.as_tensor(dy).permute(0, 3, 1, 2))
        y = E.conv2d(dev(x), dev(wt), None, dtype=dtype).cpu().numpy()
        dx, dw = E.conv2d_backward(dev(x), dev(wt), dev(dy), dtype=dtype)
        e_y = l2err(y, ref.detach().permute(0, 2, 3, 1).numpy())
        e_dx = l2err(dx.cpu().numpy(), xt.grad.permute(0, 2, 3, 1).numpy())
        e_dw = l2err(dw.cpu().numpy(), wtt.grad.permute(2, 3, 1, 0).numpy())
        gate("conv sweep y %s" % dtype, e_y, tol[0])
        gate("conv sweep dx %s" % dtype, e_dx, tol[1])
        gate("conv sweep dw %s" % dtype, e_dw, tol[1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_conv_register_filter_forms_at_other_widths(dtype):
    """conv_rf.hip (filters resident in registers, persistent workgroups over the bordered pixel space) takes the
    few-channel 3x3 launches on wide maps once the tensor is large: the multi-scale schedule feeds it widths other
    than 208 / 104 (160 ... 240, 80 ... 120), non-square maps and ragged last tiles.  Forward (with bias), dx and dW of
    the single-op entry points against torch's CPU convolution; the element-wise gate catches a misplaced tile."""
    import torch.nn.functional as F
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(77)
    #        N   H    W   Cin Cout   form exercised
    cases = [(11, 160, 160, 32, 64),    # 32 -> 64 forward (8 waves x 32 pixels x 64 couts) and its 64 -> 32 dgrad
             (5, 240, 240, 32, 64),
             (14, 120, 176, 32, 64),    # non-square
             (22, 80, 80, 64, 128),     # 64 -> 128 forward (couts over four waves)
             (10, 120, 120, 64, 128),
             (16, 104, 88, 64, 128),
             (22, 80, 80, 128, 64)]     # its plain dgrad (64 -> 128 on dy)
    tol = {"f16": 8e-4, "bf16": 6e-3}[dtype]
    for (n, h, w, ci, co) in cases:
        x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
        wt = (rng.standard_normal((3, 3, ci, co)) / np.sqrt(9 * ci)).astype(np.float32)
        b = rng.uniform(-0.5, 0.5, co).astype(np.float32)
        dy = rng.standard_normal((n, h, w, co)).astype(np.float32)
        xt = torch.as_tensor(x).permute(0, 3, 1, 2).requires_grad_(True)
        wtt = torch.as_tensor(wt).permute(3, 2, 0, 1).requires_grad_(True)
        ref = F.conv2d(xt, wtt, torch.as_tensor(b), padding=1)
        ref.backward(torch.as_tensor(dy).permute(0, 3, 1, 2))
        y = E.conv2d(dev(x), dev(wt), dev(b), dtype=dtype).cpu().numpy()
        dx, dw = E.conv2d_backward(dev(x), dev(wt), dev(dy), dtype=dtype)
        ry = ref.detach().permute(0, 2, 3, 1).numpy()
        rdx = xt.grad.permute(0, 2, 3, 1).numpy()
        gate("conv_rf y %s" % dtype, l2err(y, ry), tol)
        gate("conv_rf dx %s" % dtype, l2err(dx.cpu().numpy(), rdx), tol)
        gate("conv_rf dw %s" % dtype, l2err(dw.cpu().numpy(), wtt.grad.permute(2, 3, 1, 0).numpy()), tol)
        # a misplaced or dropped tile is a large local error that an L2 norm over 10^7 values can hide
        assert relerr(y, ry) < 20 * tol and relerr(dx.cpu().numpy(), rdx) < 20 * tol, (n, h, w, ci, co)


RF_STACKS = [
    # the second layer runs conv_rf's 32 -> 64 forward with statistics and, below a 3-channel pooled first layer
    # (no fused reduce), its 64 -> 32 dgrad with the early overflow marker's plain epilogue; width 160
    ("rf 32->64 @160", [(3, 3, 32, 1), (3, 32, 64, 1), (1, 64, 32, 0)], (11, 320, 320, 3)),
    # the second layer's dgrad (dy 64 channels -> 128) runs conv_rfn with the fused BN-backward reduce of the first
    ("rfn dgrad + reduce @104", [(1, 32, 128, 0), (3, 128, 64, 0), (1, 64, 32, 0)], (13, 104, 104, 32)),
    # conv_rfn forward with statistics at a width other than 104 (ragged last tile, 89-position rows)
    ("rfn fwd @88", [(3, 64, 128, 1), (1, 128, 32, 0)], (18, 88, 88, 64)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,spec,shape", RF_STACKS, ids=[s[0] for s in RF_STACKS])
def test_register_filter_forms_in_network(name, spec, shape):
    """The persistent register-filter kernels inside a network (f16): batch statistics from one record per
    workgroup, BN + leaky + pool, and the backward pass through their dgrad modes -- forward output and every
    parameter gradient against the float64 oracle with the same storage points quantised (as test_stack_backward)."""
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(31)
    params = _rand_params(spec, rng)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    net = E.Network(spec, shape[0], shape[1], shape[2], dtype="f16", training=True)
    net.load_params(params)
    out = net.forward(dev(x), True, True)
    q = R.quantizer("f16")
    ref, caches, _ = R.run_stack(x, params, spec, True, np.float64, quant=q)
    gate("rf stack forward f16", l2err(out.cpu().numpy(), ref), 1e-3)
    dout = rng.standard_normal(ref.shape).astype(np.float32)
    net.backward(dev(dout))
    _, rgrads = R.run_stack_backward(params, caches, dout.astype(np.float64), np.float64, quant=q,
                                     grad_scale=net.grad_scale)
    grads = net.export_grads()
    errs = {(l, k): l2err(grads[l][k], rgrads[l][k]) for l in range(len(spec)) for k in ("W", "gamma", "beta")}
    print("rf stack", name, {"%d%s" % lk: "%.1e" % v for lk, v in errs.items()})
    for (l, k), v in errs.items():
        gate("rf stack backward f16 %s" % name, v, 8e-3)     # observed 4.7e-3 (the same value with the kernels off)
    # the backward pass is deterministic (slab sums, no float atomics): repeated passes give the same bits -- a stream
    # race between the weight gradients showed up exactly here (scripts/diag_race.py)
    g0 = net.grads.clone()
    for _ in range(8):
        net.backward(dev(dout))
        torch.cuda.synchronize()
        assert torch.equal(net.grads, g0)
