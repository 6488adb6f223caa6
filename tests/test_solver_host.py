"""Darknet's SGD solver on the host (no GPU): the specification utils/solver.py -- current_rate against hand-worked
values, sgd_step against Darknet's three-call form and against the Momentum oracle -- the library's host routine
y2_solver_rate against current_rate bit for bit, the snapshot names of the Momentum slots and the solver record, and the
train script's flags."""
import ctypes as C

import numpy as np
import pytest

from oracle import optim_ref as O
from tensorflow_yolo2_amd.utils import solver as S
from tensorflow_yolo2_amd.utils import yolov2_snapshot as SN

f32, f64 = np.float32, np.float64


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def ulps(a, b):
    """distance of two float32 arrays in units of the last place (ordered-integer form, across zero too)"""
    def key(x):
        i = np.asarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


# ---------------------------------------------------------------- the schedule
def test_current_rate_hand_worked_values():
    sv = S.Solver()
    assert (sv.learning_rate, sv.momentum, sv.decay, sv.policy, sv.burn_in, sv.power, sv.steps, sv.scales,
            sv.max_batches) == (0.001, 0.9, 0.0005, "steps", 1000, 4, (40000, 60000), (0.1, 0.1), 0)
    lr, tenth = f64(f32(0.001)), f64(f32(0.1))              # the float32 constants widened, as the C ABI passes them
    expect = {1: f32(lr * 1e-12),                           # (1 / 1000)^4
              500: f32(lr * 0.0625),                        # (1 / 2)^4
              999: f32(lr * (0.999 * 0.999 * 0.999 * 0.999)),
              1000: f32(lr), 39999: f32(lr),
              40000: f32(lr * tenth), 59999: f32(lr * tenth),
              60000: f32(lr * tenth * tenth), 10 ** 6: f32(lr * tenth * tenth)}
    for t, want in expect.items():
        got = S.current_rate(sv, t)
        assert got.dtype == np.float32 and bits(got) == bits(want), (t, got, want)
    assert S.current_rate(sv, 999) < S.current_rate(sv, 1000)
    const = S.Solver(policy="constant", burn_in=0)
    assert all(bits(S.current_rate(const, t)) == bits(f32(lr)) for t in (1, 40000, 10 ** 6))
    poly = S.Solver(policy="poly", burn_in=0, max_batches=500, power=2)
    assert bits(S.current_rate(poly, 250)) == bits(f32(lr * 0.25))
    assert S.current_rate(poly, 500) == 0 and S.current_rate(poly, 501) == 0 and S.current_rate(poly, 10 ** 6) == 0
    with pytest.raises(ValueError):
        S.current_rate(sv, 0)


@pytest.mark.parametrize("field,value", [
    ("learning_rate", -1e-3), ("learning_rate", float("inf")), ("learning_rate", float("nan")),
    ("momentum", 1.0), ("momentum", -0.1), ("decay", -1e-4), ("decay", float("nan")), ("burn_in", -1),
    ("power", 0), ("power", 9), ("power", 2.5), ("policy", "exp"),
    ("steps", (0, 5)), ("steps", (5, 5)), ("steps", (7, 5)), ("steps", tuple(range(1, 10))),
    ("scales", (0.1,)), ("scales", (0.1, 0.0)), ("scales", (0.1, float("inf"))), ("max_batches", -1)])
def test_solver_validation_names_the_field(field, value):
    kw = {field: value}
    if field == "steps" and len(value) != 2:
        kw["scales"] = (0.1,) * len(value)
    with pytest.raises(ValueError, match=field):
        S.Solver(**kw)


def test_poly_needs_max_batches():
    with pytest.raises(ValueError, match="max_batches"):
        S.Solver(policy="poly")
    S.Solver(policy="poly", max_batches=1)


SOLVERS = {"steps": dict(), "steps_b0": dict(burn_in=0), "constant": dict(policy="constant"),
           "constant_b0": dict(policy="constant", burn_in=0), "poly": dict(policy="poly", max_batches=2500),
           "poly_b0": dict(policy="poly", max_batches=2500, burn_in=0, power=3),
           "three_steps": dict(steps=(1500, 2000, 2001), scales=(0.5, 3.0, 0.1), burn_in=0)}


@pytest.mark.parametrize("key", sorted(SOLVERS))
def test_library_rate_equals_current_rate_bit_for_bit(key):
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    sv = S.Solver(**SOLVERS[key])
    rec = _lib.sgd_solver(sv)
    ts = set(range(1, 3001))
    for s in sv.steps + (sv.max_batches,):
        ts |= {t for t in (s - 1, s, s + 1, s + 7) if t >= 1}
    out = C.c_float()
    for t in sorted(ts):
        assert lib.y2_solver_rate(C.byref(rec), t, C.byref(out)) == 0, t
        assert bits(out.value) == bits(S.current_rate(sv, t)), (t, out.value, S.current_rate(sv, t))


def test_library_rejects_an_invalid_record():
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    out = C.c_float()
    good = _lib.sgd_solver(S.Solver())
    assert lib.y2_solver_rate(C.byref(good), 1, C.byref(out)) == 0
    assert lib.y2_solver_rate(C.byref(good), 0, C.byref(out)) == -1          # Y2_ERR_ARG: the first applied step is 1

    def broken(**kw):
        rec = _lib.sgd_solver(S.Solver())
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(rec, k)[i] = x
            else:
                setattr(rec, k, v)
        return rec
    for kw in (dict(learning_rate=-1.0), dict(learning_rate=float("nan")), dict(momentum=1.0), dict(decay=float("inf")),
               dict(policy=3), dict(burn_in=-1), dict(power=0), dict(power=9), dict(nsteps=9), dict(steps=(5, 5)),
               dict(steps=(0, 5)), dict(scales=(0.1, 0.0)), dict(policy=2, max_batches=0)):
        assert lib.y2_solver_rate(C.byref(broken(**kw)), 1, C.byref(out)) == -1, kw
        assert b"y2_sgd_solver" in lib.y2_last_error(), kw


# ---------------------------------------------------------------- the update
def test_sgd_step_is_darknets_three_calls():
    """update_convolutional_layer on the summed gradient of a batch: wu -= decay batch w; w += lr / batch wu;
    wu *= momentum -- with acc = -wu / batch before the scal, in float64 over 20 steps"""
    rng = np.random.default_rng(0)
    n, batch, lr, mom, decay = 257, 64, 1e-3, 0.9, 5e-4
    w = rng.standard_normal(n) * 0.1
    wu = np.zeros(n)
    p, acc = w.copy(), np.zeros(n)
    for t in range(20):
        g = rng.standard_normal(n) * 1e-2                    # the mean gradient: Darknet backpropagates its sum, negated
        wu = wu - batch * g
        wu = wu - decay * batch * w
        w = w + lr / batch * wu                              # learning_rate / batch on the summed gradient
        p, acc = S.sgd_step(p, acc, g, lr, mom, decay, True, dtype=np.float64)
        assert np.abs(acc - (-wu / batch)).max() < 1e-12 and np.abs(p - w).max() < 1e-12, t
        wu = wu * mom
    assert np.abs(p - w).max() < 1e-12 and np.abs(p).max() > 1e-2


def test_sgd_step_without_decay_is_the_momentum_oracle():
    """The oracle rounds momentum * accum before it adds g, sgd_step fuses the two.  With rn() for rounding: the oracle
    gives rn(rn(m a) + g), sgd_step rn(m a + g), and |rn(m a) - m a| <= ulp(m a) / 2.
      * gradients of one sign: accum, m a and g share it, |m a| <= |result|, so the two arguments of the outer rn() lie
        within half an ulp of the RESULT and their roundings within 1 ulp -- asserted as such for accum;
      * gradients of both signs: m a and g may cancel, the result is then smaller than m a and the half ulp of m a is many
        ulps of it (908 in the second step of this stream).  What holds is 1 ulp of the LARGER of |result| and |m a|; p
        moves by the rate times that, beside its own last place."""
    rng = np.random.default_rng(1)
    lr = f32(1e-3)
    for one_sign in (True, False):
        p = (rng.standard_normal(4099) * 0.1).astype(f32)
        acc = np.zeros_like(p)
        rp, racc = p.copy(), acc.copy()
        for t in range(5):
            g = (rng.standard_normal(p.size) * 1e-2).astype(f32)
            if one_sign:
                g = np.abs(g)
            want_p, want_acc = O.momentum_step(p, acc, g, 1e-3, 0.9)
            prod = np.abs(f32(0.9) * acc)
            p, acc = S.sgd_step(p, acc, g, lr, 0.9, 0.0, True)          # decay 0: `decayed` adds a zero
            if one_sign:
                assert ulps(acc, want_acc).max() <= 1, t
                tol = np.spacing(np.abs(want_acc))
            else:
                tol = np.spacing(np.maximum(np.abs(want_acc), prod))
                assert (np.abs(acc.astype(f64) - want_acc) <= tol).all(), t
            # p = rn(p - rn(lr accum)): the rate times accum's difference, the product's and p's own last place (a p
            # near zero is not larger than its step, so "1 ulp of p" alone does not hold for it: 2 were seen)
            ptol = np.spacing(np.abs(want_p)) + np.spacing(np.abs(lr * want_acc)) + f64(lr) * tol
            assert (np.abs(p.astype(f64) - want_p) <= ptol).all(), t
            assert np.median(ulps(p, want_p)) == 0 and np.percentile(ulps(p, want_p), 99) <= 1, t
            rp, racc = S.sgd_step(rp, racc, g, lr, 0.9, 0.0005, False)  # not decayed: decay is not read
            assert np.array_equal(rp, p) and np.array_equal(racc, acc)


def test_decay_reaches_only_what_is_marked():
    p = np.array([0.5, 0.5], f32)
    q, acc = S.sgd_step(p, np.zeros(2, f32), np.zeros(2, f32), 0.1, 0.9, 0.01, np.array([True, False]))
    assert acc[0] == f32(f32(0.01) * f32(0.5)) and acc[1] == 0 and q[1] == p[1] and q[0] < p[0]


# ---------------------------------------------------------------- snapshots
def _stacks(rng):
    shapes = {"W": (3, 3, 4, 8), "b": (8,), "gamma": (8,), "beta": (8,), "moving_mean": (8,), "moving_var": (8,)}
    layer = lambda: {k: rng.standard_normal(s).astype(f32) for k, s in shapes.items()}
    stacks = {s: [layer() for _ in range(n)] for s, n in zip(SN.STACKS, (2, 1, 2))}
    slots = lambda: {s: [{k: rng.standard_normal(shapes[k]).astype(f32) for k in SN.PARAM_KEYS} for _ in stacks[s]]
                     for s in SN.STACKS}
    return stacks, slots


def test_snapshot_blob_round_trip_with_momentum_slots_and_solver_record():
    rng = np.random.default_rng(2)
    stacks, slots = _stacks(rng)
    anchors = np.asarray([[1.0, 2.0], [3.0, 4.0]], f32)
    sv = S.Solver(learning_rate=0.002, burn_in=3, steps=(3, 9), scales=(0.5, 0.25), power=2, max_batches=77)
    acc = slots()
    sgd = {s: {"accum": acc[s], "t": 41} for s in SN.STACKS}
    scaler = {"ctrl": np.arange(8, dtype=np.int32), "scale": 512.0, "clean": 7}
    blob = SN.to_blob(stacks, anchors, 20, 1234, None, scaler, sgd, sv)
    assert "yolov2/stem/1/gamma/Momentum" in blob and "yolov2/head/sgd_step" in blob
    assert not any(k.endswith("/Adam") or k.endswith("adam_step") for k in blob)
    for k in S.FIELDS:
        assert "yolov2/solver/" + k in blob, k
    assert not any(v.dtype == object for v in map(np.asarray, blob.values()))       # np.savez without pickle
    s2, an2, nc2, it2, adam2, scaler2 = SN.from_blob(blob)
    assert adam2 is None and (nc2, it2) == (20, 1234) and scaler2["clean"] == 7
    sgd2, sv2 = SN.sgd_from_blob(blob)
    assert sv2 == sv and sv2.policy == "steps" and sv2.steps == (3, 9) and sv2.max_batches == 77
    for s in SN.STACKS:
        assert sgd2[s]["t"] == 41 and len(sgd2[s]["accum"]) == len(stacks[s])
        for a, b in zip(sgd2[s]["accum"], acc[s]):
            for k in SN.PARAM_KEYS:
                assert np.array_equal(a[k], b[k])
    # the Adam names and an Adam snapshot's contents are what they were
    m, v = slots(), slots()
    adam = {s: {"m": m[s], "v": v[s], "t": 5} for s in SN.STACKS}
    ablob = SN.to_blob(stacks, anchors, 20, 1234, adam, scaler)
    assert not any("Momentum" in k or "/solver/" in k or "sgd_step" in k for k in ablob)
    assert SN.sgd_from_blob(ablob) == (None, None) and SN.from_blob(ablob)[4] is not None
    assert SN.sgd_from_blob(SN.to_blob(stacks, anchors, 20, 0)) == (None, None)
    # the mismatches: the other optimizer's slots, another solver record
    SN.check_optimizer("p.npz", True, None, None)
    SN.check_optimizer("p.npz", False, sv2, sv)
    SN.check_optimizer("p.npz", False, None, sv)             # a detector's snapshot: parameters only
    SN.check_optimizer("p.npz", False, None, None)
    with pytest.raises(ValueError, match="Momentum.*Adam"):
        SN.check_optimizer("p.npz", False, sv2, None)
    with pytest.raises(ValueError, match="Adam.*Darknet"):
        SN.check_optimizer("p.npz", True, None, sv)
    other = S.Solver(learning_rate=0.002, burn_in=3, steps=(3, 9), scales=(0.5, 0.5), power=2, max_batches=77)
    with pytest.raises(ValueError, match=r"0\.25.*0\.5"):
        SN.check_optimizer("p.npz", False, sv2, other)


# ---------------------------------------------------------------- the script's flags
def test_parse_args_solver_flags(capsys):
    from tensorflow_yolo2_amd.pascal.pascal_train_yolov2 import parse_args
    base = ["--devkit", "kit"]
    a = parse_args(base)
    assert a.solver == "adam" and a.solver_record is None
    d = parse_args(base + ["--solver", "darknet"])
    assert d.solver_record == S.Solver()
    full = parse_args(base + ["--solver", "darknet", "--lr", "0.002", "--momentum", "0.8", "--decay", "0.001", "--burn-in",
                             "100", "--power", "2", "--policy", "steps", "--steps", "400,600,900", "--scales", ".1,.5,2",
                             "--max-batches", "1000", "--box-labels", "--area-weight", "--prior-images", "12800",
                             "--multi-scale", "--augment"])
    assert full.solver_record == S.Solver(0.002, 0.8, 0.001, "steps", 100, 2, (400, 600, 900), (0.1, 0.5, 2.0), 1000)
    poly = parse_args(base + ["--solver", "darknet", "--policy", "poly", "--max-batches", "80200"])
    assert poly.solver_record.policy == "poly" and poly.solver_record.max_batches == 80200
    rejected = [["--lr", "0.002"], ["--momentum", "0.8"], ["--decay", "0.001"], ["--burn-in", "5"], ["--power", "2"],
                ["--policy", "poly"], ["--steps", "4,6"], ["--scales", ".1,.1"], ["--max-batches", "10"],
                ["--solver", "adam", "--lr", "0.002"],
                ["--solver", "sgd"],
                ["--solver", "darknet", "--steps", "400"],                     # one step, the two default scales
                ["--solver", "darknet", "--steps", "4,x"],
                ["--solver", "darknet", "--steps", "6,4", "--scales", ".1,.1"],
                ["--solver", "darknet", "--policy", "poly"],                   # poly without --max-batches
                ["--solver", "darknet", "--momentum", "1"],
                ["--solver", "darknet", "--power", "9"],
                ["--solver", "darknet", "--lr", "-1"]]
    for extra in rejected:
        with pytest.raises(SystemExit):
            parse_args(base + extra)
    capsys.readouterr()
