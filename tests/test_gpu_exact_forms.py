"""GPU tests (-m gpu): every 16-bit convolution and weight-gradient kernel form against float64, bit for bit.

tests/_exact_cases.py holds the cases and the reasoning: integer data in {-1, 0, +1}, so that every product, every
partial sum in any order and every stored value is exact in fp32, f16 and bf16.  Here engine.conv2d and
engine.conv2d_backward run each case in f16 and bf16 with the launch log on; y, dx and dW must equal the float64
reference in EVERY element (no sampling, no tolerance), and the three launches must have taken the forms the case
table pins.  Run as a script with the argument `atomic` (and Y2_NO_WGRAD_SLAB=1 set by the parent test) it runs the
float-atomics route of the weight gradients."""
import functools
import os
import subprocess
import sys

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(_HERE), _HERE]

import _exact_cases as X                                    # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _case_on_device(name):
    """(x, w, b, dy) fp32 and the float64 reference (y, dx, dW) of a case on the device, shared by its dtypes"""
    case = X.CASES[X.CASE_IDS.index(name)]
    x, w, b, dy = (torch.as_tensor(a).cuda() for a in X.case_data(case))
    y, dx, dw = X.reference(x, w, b, dy)
    X.check_magnitudes(name, y, dx, dw)          # from the reference alone, before any device value is read
    return (x, w, b, dy), (y, dx, dw)


def run_case(name, dtype, wgrad_sum=None):
    """one case through engine.conv2d / conv2d_backward with the log on: the three form keys, then every element"""
    from tensorflow_yolo2_amd import engine as E
    case = X.CASES[X.CASE_IDS.index(name)]
    (x, w, b, dy), (y_ref, dx_ref, dw_ref) = _case_on_device(name)
    assert float(y_ref.abs().max()) <= X.STORE_MAX[dtype] and float(dx_ref.abs().max()) <= X.STORE_MAX[dtype]
    E.launch_log(True)
    try:
        y = E.conv2d(x, w, b, dtype=dtype)
        dx, dw = E.conv2d_backward(x, w, dy, dtype=dtype)
        torch.cuda.synchronize()
        log = E.launch_log()
    finally:
        E.launch_log(False)
    want = X.case_keys(case, dtype)
    if wgrad_sum is not None:
        want[2] = X.wgrad_key(dtype, case[10], wgrad_sum)
    assert log == want, "%s %s took other kernel forms than the case table pins:\n  logged %s\n  pinned %s" % (
        name, dtype, [X.key_name(r) for r in log], [X.key_name(r) for r in want])
    report = [X.mismatch_report("y", y.double(), y_ref, ("image", "row", "column", "channel")),
              X.mismatch_report("dx", dx.double(), dx_ref, ("image", "row", "column", "channel")),
              X.mismatch_report("dW", dw.double(), dw_ref, ("tap row", "tap column", "ci", "co"))]
    report = [r for r in report if r]
    assert not report, "%s %s [%s]\n  " % (name, dtype, "; ".join(X.key_name(r) for r in log)) + "\n  ".join(report)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", X.CASE_IDS)
def test_op_level_forms_bit_exact(name, dtype):
    run_case(name, dtype)


def test_wgrad_float_atomics_route_bit_exact():
    """WS_ATOMIC: the library reads Y2_NO_WGRAD_SLAB once, so the route runs in a child process (this file as a script)"""
    env = dict(os.environ, Y2_NO_WGRAD_SLAB="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "atomic"], env=env, capture_output=True, text=True,
                       timeout=120)           # six small runs and the start of a process: a few seconds
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "atomic route ok" in r.stdout


# ---------------------------------------------------------------- forms only a Network launches
def _round_to(dtype):
    t = torch.float16 if dtype == "f16" else torch.bfloat16
    return lambda a: a.to(t).to(a.dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("name", X.NET_CASE_IDS)
def test_in_network_statistics_and_fused_reduce_forms(name, dtype):
    """A two-layer network in training mode, grad_scale 1.  Layer 0 holds integer filters, bias and input: its conv
    output (written by the epilogue variants that also write batch-norm records) must equal float64 at EVERY pixel, and
    the statistics the layer was normalised with must be the float64 moments of that exact output within 1e-4 of the
    largest moment.  Layer 1's dgrad carries layer 0's batch-norm-backward reduce in its epilogue: dgamma, dbeta and dy
    of layer 0 against float64 arithmetic on the values the device stored, at the gates of
    _shapes.check_layer_in_network (1e-3 of the maximum in f16; bf16: times 4, the ratio of the unit roundoffs 2^-9 and
    2^-11 -- every gated quantity is a function of values stored in the 16-bit type)."""
    import numpy as np
    from oracle import nn_ref as R
    from tensorflow_yolo2_amd import engine as E
    import _obs
    case = X.NET_CASES[X.NET_CASE_IDS.index(name)]
    _, N, H, W, (k0, cin, c1, pool), (k1, c2), seed = case[:7]
    q = _round_to(dtype)
    TOL = 1e-3 if dtype == "f16" else 4e-3
    rng = np.random.default_rng(seed + 1)
    spec = [(k0, cin, c1, pool), (k1, c1, c2, 0)]
    x, w0, b0 = X.net_case_data(case)
    params = R.init_params(spec, seed=4)
    params[0]["W"], params[0]["b"] = w0, b0
    params[1]["W"] = q(torch.as_tensor(params[1]["W"])).numpy()
    for p in params:
        p["gamma"] = rng.uniform(0.5, 1.5, p["gamma"].shape).astype(np.float32)
        p["beta"] = rng.uniform(-0.3, 0.3, p["beta"].shape).astype(np.float32)
    xd, w0d, b0d = (torch.as_tensor(a).cuda() for a in (x, w0, b0))
    y_ref = X.reference(xd, w0d, b0d, torch.zeros((N, H, W, c1), device="cuda"))[0]
    assert float(y_ref.abs().max()) <= X.STORE_MAX["bf16"], (name, float(y_ref.abs().max()))
    net = E.Network(spec, N, H, W, dtype=dtype, training=True, grad_scale=1.0)
    net.load_params(params)
    E.launch_log(True)
    try:
        out = net.forward(xd, True, True)
        dout = torch.as_tensor(rng.uniform(-1, 1, tuple(out.shape)).astype(np.float32)).cuda()
        net.backward(dout)
        torch.cuda.synchronize()
        log = E.launch_log()
    finally:
        E.launch_log(False)
    want_fwd, want_dgrad = X.net_case_keys(case, dtype)
    names = [X.key_name(r) for r in log]
    assert want_fwd in log and want_dgrad in log, "%s %s: pinned %s and %s, logged %s" % (
        name, dtype, X.key_name(want_fwd), X.key_name(want_dgrad), names)
    # ---- layer 0's conv output, every pixel, and its statistics
    y = net.debug_read(0, 1).double()
    msg = X.mismatch_report("y", y, y_ref, ("image", "row", "column", "channel"))
    assert not msg, "%s %s [%s] %s" % (name, dtype, X.key_name(want_fwd), msg)
    st = net.layer_statistics(0)
    mean, var = y_ref.mean((0, 1, 2)), y_ref.var((0, 1, 2), unbiased=False)
    e_m = float((torch.as_tensor(st["mean"]).cuda() - mean).abs().max() / max(float(mean.abs().max()), float(var.max().sqrt())))
    e_v = float((torch.as_tensor(st["var"]).cuda() - var).abs().max() / var.max())
    _obs.gate("exact net %s %s batch mean" % (name, dtype), e_m, 1e-4)
    _obs.gate("exact net %s %s batch variance" % (name, dtype), e_v, 1e-4)
    # ---- layer 1's dgrad + the fused reduce: dA from layer 1's stored dy and filters, then BN / leaky / pool backward
    g = net.export_grads()
    gamma = torch.as_tensor(params[0]["gamma"]).cuda().double()
    beta = torch.as_tensor(params[0]["beta"]).cuda().double()
    dy1 = net.debug_read(1, 2)
    dA = q(X.dgrad_reference(dy1, torch.as_tensor(params[1]["W"]).cuda()).float()).double()      # stored in the 16-bit type
    inv = 1.0 / torch.sqrt(var + 1e-3)
    xhat = (y_ref - mean) * inv
    z = xhat * gamma + beta
    act = torch.maximum(0.1 * z, z)
    near = z.abs() < 1e-4
    if pool:
        Ho, Wo = H // 2, W // 2
        win = lambda t: t.reshape(N, Ho, 2, Wo, 2, c1).permute(0, 1, 3, 2, 4, 5).reshape(N, Ho, Wo, 4, c1)
        unwin = lambda t: t.reshape(N, Ho, Wo, 2, 2, c1).permute(0, 1, 3, 2, 4, 5).reshape(N, H, W, c1)
        wz = win(act)
        # the device takes the FIRST maximum in row-major window order; integer conv outputs tie often
        slot = torch.arange(4, device="cuda").reshape(1, 1, 1, 4, 1)
        first = torch.where(wz == wz.max(3, keepdim=True).values, slot, 4).min(3, keepdim=True).values
        dact = unwin((slot == first).double() * dA.unsqueeze(3))
        top2 = wz.topk(2, dim=3).values
        gap = top2[:, :, :, 0] - top2[:, :, :, 1]
        near_w = win(near.double()).amax(3).bool() | ((gap < 1e-4) & (gap > 0))      # an exact tie is no decision
        near = unwin(near_w.unsqueeze(3).expand(-1, -1, -1, 4, -1).double()).bool()
    else:
        dact = dA
    dz = dact * torch.where(0.1 * z >= z, 0.1, 1.0)
    M = N * H * W
    dbeta, dgamma = dz.sum((0, 1, 2)), (dz * xhat).sum((0, 1, 2))
    dy_ref = gamma * inv * (dz - dbeta / M - xhat * dgamma / M)
    dy = net.debug_read(0, 2).double()
    bad = (dy - dy_ref).abs() > TOL * dy_ref.abs().max()
    nbad = int(bad.sum())
    assert nbad <= 8 + 2e-7 * dy.numel(), (name, dtype, "too many dy entries off", nbad)
    assert not bool((bad & ~near).any()), (name, dtype, "a dy entry is off away from any decision boundary")
    e_dy = float((torch.where(bad, dy_ref, dy) - dy_ref).abs().max() / dy_ref.abs().max())
    flip = nbad * 2.0 * float(dA.abs().max())
    e_dg = max(0.0, float((torch.as_tensor(g[0]["gamma"]).cuda() - dgamma).abs().max()) - flip * float(xhat.abs().max())) \
        / float(dgamma.abs().max())
    e_db = max(0.0, float((torch.as_tensor(g[0]["beta"]).cuda() - dbeta).abs().max()) - flip) / float(dbeta.abs().max())
    print("exact net %s %s [%s | %s]: mean %.2e var %.2e  dy %.2e (%d near-tie flips) dgamma %.2e dbeta %.2e" % (
        name, dtype, X.key_name(want_fwd), X.key_name(want_dgrad), e_m, e_v, e_dy, nbad, e_dg, e_db))
    _obs.gate("exact net %s fused reduce dy" % dtype, e_dy, TOL)
    _obs.gate("exact net %s fused reduce dgamma" % dtype, e_dg, TOL)
    _obs.gate("exact net %s fused reduce dbeta" % dtype, e_db, TOL)


# (tag, N, k, cin, cout, hw, pool, forward apply route, backward apply route) of csrc/net.hip plan_net.  The routes
# follow from two record counts and the width: the forward pass merges its statistics inside the apply kernel
# (FA_FIN_ACT, bn_fin_act) when layer 0's forward wrote P <= 128 records and cout is a multiple of 64, else it runs
# bn_finalize + bn_act (FA_ACT); the backward pass likewise (BA_FIN_APPLY against BA_FIN_THEN_APPLY) on the bP records of
# the fused dgrad.  P = ceil(N hw^2 / pixels of the forward tile), bP = ceil(pixels of layer 1 / pixels of the dgrad
# tile); the tiles are read from the log, the counts asserted, so a policy edit that moves a shape to the other route
# fails here.
NET_ROUTES = [("short lists", 2, 3, 32, 128, 12, 0, "FA_FIN_ACT", "BA_FIN_APPLY"),
              ("short lists, pooled", 2, 3, 32, 64, 12, 1, "FA_FIN_ACT", "BA_FIN_APPLY"),
              ("short lists, 1x1", 4, 1, 64, 128, 10, 0, "FA_FIN_ACT", "BA_FIN_APPLY"),
              ("256 records", 8, 1, 128, 128, 64, 0, "FA_ACT", "BA_FIN_THEN_APPLY"),
              ("544 and 136 records, pooled", 17, 1, 64, 128, 64, 1, "FA_ACT", "BA_FIN_THEN_APPLY"),
              ("160 and 40 records, pooled", 5, 1, 64, 128, 64, 1, "FA_ACT", "BA_FIN_APPLY"),
              ("72 and 144 records", 9, 3, 64, 64, 64, 0, "FA_FIN_ACT", "BA_FIN_THEN_APPLY"),
              ("32 channels", 2, 3, 64, 32, 12, 0, "FA_ACT", "BA_FIN_THEN_APPLY")]
BN_FIN_PMAX, BN_SLAB = 128, 64           # csrc/kernels.h kBnFinPmax, kBnSlab


def _tile_pixels(rec):
    """pixels per batch-norm record of a logged convolution (not the register-filter kinds: one record per workgroup)"""
    assert rec[3] not in (X.CK_RF, X.CK_RFN)
    return 128 if rec[5] else (rec[4] & 15) * ((rec[4] >> 8) & 15) * 32


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("tag,N,k,cin,cout,hw,pool,apply,bapply", NET_ROUTES,
                         ids=[s[0].replace(" ", "_").replace(",", "") for s in NET_ROUTES])
def test_layer_in_network_bn_passes_f16_and_bf16(tag, N, k, cin, cout, hw, pool, apply, bapply, dtype):
    """_shapes.check_layer_in_network (general values, float64 on what the device stored: statistics, BN + leaky (+ pool)
    output, dy, dgamma, dbeta, dW) in both 16-bit types at every forward / backward apply route of plan_net, pooled and
    not: the batch-norm kernels <bf16_t> at the gates of the f16 ones times 4 (unit roundoff 2^-9 against 2^-11), with
    the log showing that the dgrad which fed them was the fused form and the record counts that select the route"""
    from tensorflow_yolo2_amd import engine as E
    from _shapes import TOL, check_layer_in_network
    E.launch_log(True)
    try:
        check_layer_in_network(N, tag, k, cin, cout, hw, pool, tag="exact-forms", dtype=dtype,
                               TOL=TOL if dtype == "f16" else 4 * TOL)
        log = E.launch_log()
    finally:
        E.launch_log(False)
    fused = [r for r in log if r[0] == 0 and r[2] == 1 and r[6] == X.EPI_BNBWD]
    assert len(fused) == 1 and fused[0][1] == X.LAUNCH_DTYPE[dtype], [X.key_name(r) for r in log]
    fwd = [r for r in log if r[0] == 0 and r[2] == 0 and r[6] == X.EPI_STATS]
    assert len(fwd) == 2, [X.key_name(r) for r in log]          # layer 0, then layer 1
    M0, M1 = N * hw * hw, N * (hw // 2 if pool else hw) ** 2
    P = -(-M0 // _tile_pixels(fwd[0]))
    bP = -(-M1 // _tile_pixels(fused[0]))
    wide = cout % BN_SLAB == 0
    got = ("FA_FIN_ACT" if P <= BN_FIN_PMAX and wide else "FA_ACT",
           "BA_FIN_APPLY" if bP <= BN_FIN_PMAX and wide else "BA_FIN_THEN_APPLY")
    print("route %s %s: P = %d, bP = %d, cout = %d -> %s, %s" % (tag, dtype, P, bP, cout, got[0], got[1]))
    assert got == (apply, bapply), (tag, P, bP, got)


# ---------------------------------------------------------------- the universe: every form the shipped graphs launch
def _pinned_keys(dtype):
    keys = set()
    for case in X.CASES:
        keys.update(X.case_keys(case, dtype))
    for case in X.NET_CASES:
        keys.update(X.net_case_keys(case, dtype))
    return keys


# form keys a shipped graph launches that no exact case pins: empty, and it stays empty
UNCOVERED_ALLOWED = set()


def _graphs():
    """(name, one step of the graph): the five configurations of BASELINE.json, the ResNet-50 swap, the yolov2-voc and
    tiny-yolo-voc Darknet topologies, single-image detection -- at their real geometry, f16"""
    import numpy as np
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.trainer import ClassifierTrainer, DetectorTrainer, MultiScaleDetectorTrainer
    from tensorflow_yolo2_amd.yolo2_nets import tf_resnet, yolov2
    dev = lambda a: torch.as_tensor(a).cuda()
    pixels = lambda n, size: dev(np.random.default_rng(0).integers(0, 256, (n, size, size, 3), dtype=np.uint8))

    def truth(n, size):
        t = np.zeros((n, 30, 5), np.float32)
        t[:, 0] = (0.33 * size, 0.4 * size, 0.36 * size, 0.45 * size, 3)
        t[:, 1] = (0.69 * size, 0.6 * size, 0.31 * size, 0.28 * size, 7)
        return dev(t), dev(np.full(n, 2, np.int32))

    def detect(n, size):                      # configs[0] (one image) and configs[1] (batch 32): inference
        net = E.Network(list(E.CORE_SPEC) + E.det_head_spec(30), n, size, size, dtype="f16", core_layers=18, training=False)
        net.init_params(0)
        net.forward(dev(synthetic.images(n, size, 1)), False, False)

    def detector_step(n, size, dtype="f16"):  # configs[3]
        tr = DetectorTrainer(n, size, dtype=dtype, seed=0)
        tr.step(dev(synthetic.images(n, size, 1234)), dev(synthetic.det_labels(n, size, size // 32, 4321)))

    def classifier_step():                    # configs[2]
        tr = ClassifierTrainer(128, 224, dtype="f16", seed=0)
        tr.step(dev(synthetic.images(128, 224, 1)), dev(np.arange(128, dtype=np.int32) % 1000))

    def multi_scale_steps():                  # configs[4]
        ms = MultiScaleDetectorTrainer(16, sizes=(320, 608), period=1, dtype="f16", seed=0)
        for size in (320, 608):
            ms.step(dev(synthetic.images(16, size, 1)), dev(synthetic.det_labels(16, size, size // 32, 2)))

    def resnet_step():
        m = tf_resnet.ResNet50Yolo(4, 224, dtype="f16", seed=0)
        m.step(dev(synthetic.images(4, 224, 1)), dev(synthetic.det_labels(4, 224, 7, 2)))

    def darknet_step(topology, anchors):
        tr = yolov2.YOLOv2DarknetTrainer(8, 416, num_class=20, anchors=anchors, dtype="f16", seed=0, topology=topology)
        t, nt = truth(8, 416)
        tr.step(pixels(8, 416), truth=t, ntruth=nt)

    def darknet_detect():
        d = yolov2.YOLOv2Detector(1, 416, num_class=20, dtype="f16", seed=0, topology="darknet")
        d.detect(pixels(1, 416))

    return [("detect one image", lambda: detect(1, 416)), ("core forward 416 bs32", lambda: detect(32, 416)),
            ("classifier 224 bs128", classifier_step), ("detector 416 bs64", lambda: detector_step(64, 416)),
            ("multi-scale 320+608 bs16", multi_scale_steps), ("resnet50 224 bs4", resnet_step),
            ("yolov2-voc 416 bs8", lambda: darknet_step("darknet", yolov2.ANCHORS_VOC)),
            ("tiny-yolo-voc 416 bs8", lambda: darknet_step("tiny", yolov2.ANCHORS_TINY_VOC)),
            ("yolov2-voc detect one image", darknet_detect),
            ("detector 320 bs4", lambda: detector_step(4, 320)), ("detector 320 bs4 bf16", lambda: detector_step(4, 320, "bf16"))]


def _logged_forms(step):
    from tensorflow_yolo2_amd import engine as E
    E.launch_log(True)
    try:
        step()
        torch.cuda.synchronize()
        return E.launch_log()
    finally:
        E.launch_log(False)
        torch.cuda.empty_cache()


def test_every_form_the_shipped_graphs_launch_is_pinned_by_an_exact_case():
    """No reference arithmetic: one step of each shipped graph with the log on.  Every 16-bit form key must be pinned by
    an exact case above; the table of forms and the graphs that launch each is printed (profiles/exact_forms.txt)."""
    pinned = {"f16": _pinned_keys("f16"), "bf16": _pinned_keys("bf16")}
    table, small = {}, {}
    for name, step in _graphs():
        for rec in _logged_forms(step):
            if rec[1] not in (1, 2):
                continue                    # launches of the first-layer modes' fp32 / split types: out of scope
            dtype = "f16" if rec[1] == 1 else "bf16"
            if name.startswith("detector 320"):
                small.setdefault(dtype, set()).add(rec[:1] + rec[2:])
            if dtype == "f16":
                table.setdefault(rec, []).append(name)
            assert rec in pinned[dtype] or rec in UNCOVERED_ALLOWED, \
                "%s launches a form no exact case pins: %s %s" % (name, X.key_name(rec), rec)
    # f16 and bf16 take identical plans: the smallest graph logs the same keys in both types
    assert small["f16"] == small["bf16"] and small["f16"]
    print("\nFORMS Kernel forms of the 16-bit convolutions and weight gradients: the exact cases that pin each form key and")
    print("FORMS the shipped graphs that launch it (python -m pytest tests/test_gpu_exact_forms.py -m gpu -s -k every_form;")
    print("FORMS the lines that begin with FORM).  Key: the launch log of csrc/kernels.h; f16 shown, bf16 takes the same plans.")
    print("FORMS %d keys pinned, %d launched by a shipped graph, %d of those pinned by no case" % (
        len(pinned["f16"]), len(table), len(set(table) - pinned["f16"])))
    print("FORMS form key                                             exact cases   graphs")
    for rec in sorted(pinned["f16"] | set(table)):
        cases = [c[0] for c in X.CASES if rec in X.case_keys(c, "f16")] + \
                [c[0] for c in X.NET_CASES if rec in X.net_case_keys(c, "f16")]
        print("FORM %-52s %2d case(s)   %s" % (X.key_name(rec), len(cases),
                                               ", ".join(dict.fromkeys(table.get(rec, []))) or "(no shipped graph)"))
    assert not UNCOVERED_ALLOWED


if __name__ == "__main__":
    assert sys.argv[1:] == ["atomic"] and os.environ.get("Y2_NO_WGRAD_SLAB")
    for case_name in X.ATOMIC_CASES:
        for dt in ("f16", "bf16"):
            run_case(case_name, dt, wgrad_sum=X.WS_ATOMIC)
    print("atomic route ok")
