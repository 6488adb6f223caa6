"""Darknet's SGD solver on the GPU (-m gpu): y2_sgd_step (the flat kernel of csrc/optim.hip) and y2_sgd_step_packed (KIND 2
of csrc/pack.hip's fused update + re-pack) against the specification utils/solver.py, against each other bit for bit and
against MomentumOptimizer at decay 0; the overflow guard and the device-side rate schedule; YOLOv2Trainer(solver=...) and
pascal_train_yolov2 --solver darknet with its resume.

One small stack has every path of the kernels: a 3-channel first filter (a small range that decays), a 32 -> 96 filter
(tail tiles: Cout is no multiple of 64; 27,648 elements: seven blocks of the flat kernel, the last one partial) and a
1x1 output convolution to 125 channels (Cout % 4 != 0: the scalar path of the tiles, and a 375-element last segment
whose end is not 16-byte aligned).

Why 1 ulp and not 0 against the specification: numpy has no fused multiply-add, so the specification's fma goes through
float64 and may double-round.  That moves accum by at most 1 ulp, and p, which subtracts a much smaller product, by at
most 1."""
import os

import numpy as np
import pytest
import torch

from test_box_list_host import build_devkit
from test_solver_host import bits, ulps
from tensorflow_yolo2_amd.utils import solver as S

pytestmark = pytest.mark.gpu
SPEC = [(3, 3, 32, 1), (3, 32, 96, 0), (1, 96, 125, 0)]
N, SIZE = 2, 32
RAMP = dict(burn_in=3, steps=(3,), scales=(0.5,))          # rates lr/81, 16 lr/81, then lr/2: every step another one


def make(dtype, seed=5):
    from tensorflow_yolo2_amd import engine as E
    net = E.Network(SPEC, N, SIZE, SIZE, dtype=dtype, training=True)
    net.init_params(seed)
    return net


def host(t):
    return t.detach().cpu().numpy().copy()


def lr_word(scaler):
    """the control block's lr_t as its 32 bits"""
    return scaler.ctrl.cpu().numpy().view(np.uint32)[4]


def gradient(rng, n):
    return (rng.standard_normal(n) * 1e-2).astype(np.float32)


def spec_step(opt, p, acc, g, rate, grad_mult=1.0):
    mask = S.network_decayed(opt.net)
    sv = opt.solver
    return S.sgd_step(p, acc, (g * np.float32(grad_mult)).astype(np.float32), rate, sv.momentum, sv.decay, mask)


# ---------------------------------------------------------------- 1. the flat form against the specification
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_flat_step_matches_the_specification(dtype):
    from tensorflow_yolo2_amd import engine as E
    net = make(dtype)
    sv = S.Solver(**RAMP)
    assert sv.decay == 0.0005
    opt = E.DarknetSGD(net, sv, fused_pack=False)
    assert opt.guard == (dtype == "f16")
    mask = S.network_decayed(net)
    rng = np.random.default_rng(0)
    grads = [gradient(rng, net.n_params) for _ in range(3)]
    # on the CPU first: this test can tell which tensors decay.  The specification with every tensor decayed, and with
    # none, each leave the right one by more than 100 ulps of accum -- the first in a gamma / beta tensor, the second in
    # every filter, the 3-channel one included
    p0 = host(net.params)
    chains = {}
    for name, m in (("right", mask), ("all", np.ones_like(mask)), ("none", np.zeros_like(mask))):
        p, acc = p0.copy(), np.zeros_like(p0)
        for t, g in enumerate(grads, 1):
            p, acc = S.sgd_step(p, acc, g, S.current_rate(sv, t), sv.momentum, sv.decay, m)
        chains[name] = acc
    offs = [net._offsets[l] for l in range(net.num_layers)]
    ends = [o[0] for o in offs[1:]] + [net.n_params]
    d_all, d_none = ulps(chains["all"], chains["right"]), ulps(chains["none"], chains["right"])
    assert max(d_all[o[2]:e].max() for o, e in zip(offs, ends)) > 100            # gamma / beta of some layer
    assert all(d_all[o[0]:o[1]].max() == 0 for o in offs)
    assert all(d_none[o[0]:o[1]].max() > 100 for o in offs) and offs[0][1] - offs[0][0] == 27 * 32
    assert all(d_none[o[1]:e].max() == 0 for o, e in zip(offs, ends))
    # the device, step by step from its own state
    for t, g in enumerate(grads, 1):
        p, acc = host(net.params), host(opt.accum)
        net.grads.copy_(torch.as_tensor(g))
        opt.step(full_check=True)
        want_p, want_acc = spec_step(opt, p, acc, g, S.current_rate(sv, t))
        da, dp = ulps(host(opt.accum), want_acc), ulps(host(net.params), want_p)
        print("flat %s step %d: accum within %d ulp, params within %d ulp" % (dtype, t, da.max(), dp.max()))
        assert da.max() <= 1 and dp.max() <= 1, t
        assert not np.array_equal(host(net.params), p)
    if opt.guard:
        assert opt.scaler.state() == (0, 3, 0) and lr_word(opt.scaler) == bits(S.current_rate(sv, 3))


# ---------------------------------------------------------------- 2. packed equals flat
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16", "f16x2"])
def test_packed_step_equals_flat_step_bit_for_bit(dtype):
    from tensorflow_yolo2_amd import engine as E, synthetic
    x = torch.as_tensor(synthetic.images(N, SIZE, 3)).cuda()
    sv = S.Solver(**RAMP)
    nets = [make(dtype), make(dtype)]
    opts = [E.DarknetSGD(net, sv, guard=False, fused_pack=fused) for net, fused in zip(nets, (True, False))]
    rng = np.random.default_rng(0)
    for step in range(3):
        g = torch.as_tensor(gradient(rng, nets[0].n_params)).cuda()
        outs = []
        for net, opt in zip(nets, opts):
            net.grads.copy_(g)
            opt.step()
            outs.append(net.forward(x, True, True).clone())          # the flat step left its packed copies stale
        assert torch.equal(nets[0].params, nets[1].params), step
        assert torch.equal(opts[0].accum, opts[1].accum), step
        assert torch.equal(outs[0], outs[1]), step
    assert float(opts[0].accum.abs().max()) > 0


# ---------------------------------------------------------------- 3. without decay and schedule: MomentumOptimizer
@pytest.mark.parametrize("fused", [True, False])
def test_without_decay_and_schedule_it_is_the_momentum_optimizer(fused):
    from tensorflow_yolo2_amd import engine as E
    sv = S.Solver(decay=0.0, policy="constant", burn_in=0)
    a, b = make("f32"), make("f32")
    sgd = E.DarknetSGD(a, sv, guard=False, fused_pack=fused)
    mom = E.MomentumOptimizer(b, 1e-3, 0.9, guard=False, fused_pack=fused)
    rng = np.random.default_rng(1)
    for step in range(3):
        g = torch.as_tensor(gradient(rng, a.n_params)).cuda()
        for net, opt in ((a, sgd), (b, mom)):
            net.grads.copy_(g)
            opt.step()
        assert torch.equal(a.params, b.params) and torch.equal(sgd.accum, mom.accum), step


# ---------------------------------------------------------------- 4. the guard
@pytest.mark.parametrize("fused", [True, False])
def test_overflow_skips_the_step_and_the_schedule(fused):
    from tensorflow_yolo2_amd import engine as E, synthetic
    x = torch.as_tensor(synthetic.images(N, SIZE, 3)).cuda()
    net = make("f16")
    sv = S.Solver(burn_in=50)
    opt = E.DarknetSGD(net, sv, fused_pack=fused)
    assert opt.guard
    rng = np.random.default_rng(2)
    net.grads.copy_(torch.as_tensor(gradient(rng, net.n_params)))
    opt.step(full_check=True)
    assert opt.scaler.state() == (0, 1, 0) and lr_word(opt.scaler) == bits(S.current_rate(sv, 1))
    before = (net.params.clone(), opt.accum.clone(), net.forward(x, True, True).clone())
    g = gradient(rng, net.n_params)
    g[g.size // 2] = np.inf
    net.grads.copy_(torch.as_tensor(g))
    opt.step(full_check=True)
    assert opt.scaler.state() == (1, 1, 1) and lr_word(opt.scaler) == bits(S.current_rate(sv, 1))
    assert torch.equal(net.params, before[0]) and torch.equal(opt.accum, before[1])
    assert torch.equal(net.forward(x, True, True), before[2])
    # the next clean step is step 2, at the rate of step 2
    g = gradient(rng, net.n_params)
    net.grads.copy_(torch.as_tensor(g))
    opt.step(full_check=True)
    assert bits(S.current_rate(sv, 2)) != bits(S.current_rate(sv, 1)) != bits(S.current_rate(sv, 3))
    assert opt.scaler.state() == (0, 2, 1) and lr_word(opt.scaler) == bits(S.current_rate(sv, 2))
    want_p, want_acc = spec_step(opt, host(before[0]), host(before[1]), g, S.current_rate(sv, 2))
    assert ulps(host(opt.accum), want_acc).max() <= 1 and ulps(host(net.params), want_p).max() <= 1


# ---------------------------------------------------------------- 5. the schedule on the device
def test_device_schedule_equals_current_rate_bit_for_bit():
    from tensorflow_yolo2_amd import engine as E
    net = E.Network([(3, 32, 32, 0)], 1, 8, 8, dtype="f16", training=True)
    net.init_params(1)
    net.grads.zero_()
    zeros = np.zeros(net.n_params, np.float32)
    sv = S.Solver()
    cases = [(sv, t) for t in (1, 2, sv.burn_in - 1, sv.burn_in, sv.burn_in + 1, sv.steps[0] - 1, sv.steps[0],
                               sv.steps[1], sv.steps[1] + 7)]
    poly = S.Solver(policy="poly", max_batches=500, burn_in=100, power=3)
    cases += [(poly, t) for t in (99, 100, 250, 499, 500, 501)]
    const = S.Solver(policy="constant", burn_in=0)
    cases += [(const, 1), (const, 123456)]
    opts = {}
    for s, t in cases:
        opt = opts.setdefault(id(s), E.DarknetSGD(net, s))
        opt.load_state({"accum": zeros, "t": t - 1})
        opt.step(full_check=True)
        found, step, _ = opt.scaler.state()
        assert (found, step) == (0, t)
        assert lr_word(opt.scaler) == bits(S.current_rate(s, t)), (s, t)
    assert S.current_rate(poly, 500) == 0 and S.current_rate(sv, 40000) < S.current_rate(sv, 39999)


# ---------------------------------------------------------------- 6. the composed trainer
def two_objects(n, size):
    """a box list with two objects per image"""
    truth = np.zeros((n, 30, 5), np.float32)
    for i in range(n):
        truth[i, 0] = (1.3 * 32, 1.6 * 32, 45.0, 58.0, 3 + i)
        truth[i, 1] = (1.7 * 32, 1.4 * 32, 40.0, 36.0, 9 + i)
    return truth, np.full(n, 2, np.int32)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_trainer_steps_follow_the_specification(dtype):
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, size = 2, 96
    sv = S.Solver(**RAMP)
    tr = yolov2.YOLOv2Trainer(n, size, dtype=dtype, seed=3, width_div=8, solver=sv)
    assert all(isinstance(o, E.DarknetSGD) for o in tr.opts) and tr.solver is sv
    scaler = tr.opts[0].scaler
    assert (scaler is not None) == (dtype == "f16") and all(o.scaler is scaler for o in tr.opts)
    x = torch.as_tensor(synthetic.images(n, size, 31)).cuda()
    truth, ntruth = two_objects(n, size)
    td, cd = torch.as_tensor(truth).cuda(), torch.as_tensor(ntruth).cuda()
    applied = 0
    for it in range(5 if dtype == "f16" else 4):
        overflow = dtype == "f16" and it == 2
        if overflow:
            scaler._apply(2.0 ** 40)
        before = [(host(net.params), host(opt.accum)) for net, opt in zip(tr.nets, tr.opts)]
        loss = tr.step(x, truth=td, ntruth=cd)
        torch.cuda.synchronize()
        if overflow:
            assert scaler.state() == (1, applied, 1)
            assert not all(bool(torch.isfinite(net.grads).all()) for net in tr.nets)
            for (p, acc), net, opt in zip(before, tr.nets, tr.opts):
                assert np.array_equal(host(net.params), p) and np.array_equal(host(opt.accum), acc)
            scaler._apply(1024.0)
            continue
        applied += 1
        rate = S.current_rate(sv, applied)
        if scaler is not None:
            assert scaler.state()[:2] == (0, applied) and lr_word(scaler) == bits(rate)
        assert np.isfinite(float(loss[4]))
        for (p, acc), net, opt in zip(before, tr.nets, tr.opts):
            want_p, want_acc = spec_step(opt, p, acc, host(net.grads), rate)
            assert ulps(host(opt.accum), want_acc).max() <= 1 and ulps(host(net.params), want_p).max() <= 1, (it, applied)
            assert not np.array_equal(host(net.params), p)
    assert applied == 4 and bits(S.current_rate(sv, 4)) == bits(np.float32(np.float32(0.001) * np.float64(np.float32(0.5))))
    for net in tr.nets:
        assert torch.isfinite(net.params).all()


def test_trainer_without_a_solver_is_the_adam_trainer():
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, size = 2, 96
    x = torch.as_tensor(synthetic.images(n, size, 31)).cuda()
    truth, ntruth = two_objects(n, size)
    td, cd = torch.as_tensor(truth).cuda(), torch.as_tensor(ntruth).cuda()
    a = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=3, width_div=8, solver=None)
    b = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=3, width_div=8)
    assert a.solver is None and all(type(o) is E.AdamOptimizer for o in a.opts + b.opts)
    for it in range(2):
        la, lb = a.step(x, truth=td, ntruth=cd), b.step(x, truth=td, ntruth=cd)
        assert torch.equal(la, lb)
        for na, nb, oa, ob in zip(a.nets, b.nets, a.opts, b.opts):
            assert torch.equal(na.params, nb.params) and torch.equal(oa.m, ob.m) and torch.equal(oa.v, ob.v), it
    assert a.opts[0].scaler.state() == b.opts[0].scaler.state() == (0, 2, 0)


# ---------------------------------------------------------------- 7. the script and its resume
def _train(kit, ckpt, iters, solver=True):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2
    flags = ["--solver", "darknet", "--burn-in", "3", "--steps", "3", "--scales", ".5"] if solver else []
    return pascal_train_yolov2.main(["--devkit", kit, "--ckpt-dir", ckpt, "--box-labels", "--augment", "--width-div", "8",
                                     "--batch", "2", "--size", "96", "--iters", str(iters)] + flags)


def _differing(a, b):
    assert sorted(a.files) == sorted(b.files)
    return [k for k in a.files if a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]


def test_train_script_resumes_bitwise_on_the_darknet_solver(tmp_path, golden_dir):
    """4 iterations in one run against 2, a snapshot, a fresh process state from --ckpt-dir and 2 more: the schedule leaves
    its burn-in and takes its step (both at 3) inside the resumed half.  A second uninterrupted run is the control."""
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    dirs = [str(tmp_path / d) for d in ("whole", "control", "resumed")]
    whole = _train(kit, dirs[0], 4)
    _train(kit, dirs[1], 4)
    first = _train(kit, dirs[2], 2)
    second = _train(kit, dirs[2], 2)
    assert (first["first_iter"], first["last_iter"], second["first_iter"], second["last_iter"]) == (1, 2, 3, 4)
    sv = S.Solver(**RAMP)
    assert whole["trainer"].solver == sv
    losses = np.array(whole["losses"])
    assert losses.shape == (4, 5) and np.isfinite(losses).all()
    paths = [os.path.join(d, "train_iter_4.npz") for d in dirs]
    snaps = [np.load(p) for p in paths]
    assert "yolov2/stem/0/W/Momentum" in snaps[0].files and int(snaps[0]["yolov2/head/sgd_step"]) == 4
    assert not any(k.endswith("/Adam") for k in snaps[0].files)
    ctrl = snaps[0]["yolov2/scaler/ctrl"]
    assert ctrl[1] == 4 and ctrl[2] == 0 and ctrl.view(np.uint32)[4] == bits(S.current_rate(sv, 4))
    assert float(np.abs(snaps[0]["yolov2/deep/0/W/Momentum"]).max()) > 0
    assert _differing(snaps[0], snaps[1]) == [], "the uninterrupted run is not reproducible itself"
    assert _differing(snaps[0], snaps[2]) == []
    assert np.array_equal(np.array(first["losses"] + second["losses"]).view(np.uint32), losses.view(np.uint32))
    # each optimizer restores its own slots only
    n_class, anchors = whole["trainer"].num_class, whole["anchors"]
    adam = yolov2.YOLOv2Trainer(2, 96, num_class=n_class, anchors=anchors, width_div=8)
    with pytest.raises(ValueError, match="Momentum.*Adam"):
        net_utils.restore_yolov2_variables(adam, paths[0])
    adam_path = str(tmp_path / "adam.npz")
    net_utils.save_yolov2_variables(adam, adam_path)
    with pytest.raises(ValueError, match="Adam.*Darknet"):
        net_utils.restore_yolov2_variables(second["trainer"], adam_path)
    other = yolov2.YOLOv2Trainer(2, 96, num_class=n_class, anchors=anchors, width_div=8, solver=S.Solver(burn_in=3))
    with pytest.raises(ValueError, match="solver record"):
        net_utils.restore_yolov2_variables(other, paths[0])
    # a detector takes the parameters of either kind
    det = yolov2.YOLOv2Detector(2, 96, num_class=n_class, anchors=anchors, width_div=8)
    assert net_utils.restore_yolov2_variables(det, paths[0]) == 4
    assert torch.equal(det.stem.params, second["trainer"].nets[0].params)
    assert net_utils.restore_yolov2_variables(det, adam_path) == 0
