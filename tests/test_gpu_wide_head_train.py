"""Training the wide head on the GPU (csrc/wide_head_train.hip): the two backward products and the bias gradient against
numpy float64 on the operands as the kernels round them, every split count the plan can return, the overflow scan, the
solver step and both packed images, the argument errors, and YOLOv2DarknetTrainer.from_cfg(..., wide_head=True) on
tests/golden/cfg/chain-wide.cfg through a step, a second input size and a `.weights` round trip.

Product parity.  With f16(x), f16(W) and f16(s dy) the products are exact in fp32, so only the accumulation order differs
from the reference: per element |got - ref| <= 2 R 2^-24 sum |a b| / s + 1e-30, R the reduction length (Cout for dx, M for
dW) -- the forward test's bound.  db is an fp32 sum of M unconverted values: 2 M 2^-24 sum |dy|."""
import ctypes

import numpy as np
import pytest

import _wide_head_cases as K
from test_solver_host import ulps
from tensorflow_yolo2_amd.utils import solver as S

pytestmark = pytest.mark.gpu
GUARD = K.GUARD
SHAPES = ((1, 64, 1), (25, 32, 225), (256, 64, 256), (257, 64, 257), (513, 96, 300), (40, 1024, 515), (147, 128, 2115),
          (300, 256, 28269))
PLAN_CUS = range(1, 1025)            # the compute-unit counts the plan is enumerated over: every part up to 1,024 CUs


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def host(t):
    return t.detach().cpu().numpy().copy()


def _lib():
    from tensorflow_yolo2_amd import _lib as L
    return L.load()


def gradient(M, Cout, seed=0):
    """dy [M][Cout] float32: mixed signs, a spread of row magnitudes, times 1,024 still far inside f16"""
    rng = np.random.default_rng(7919 * M + Cout + seed)
    return (rng.standard_normal((M, Cout)) * 0.05 * np.exp(rng.uniform(-2, 2, (M, 1)))).astype(np.float32)


def plan_splits(lib, M, Kdim, Cout):
    """-> (every dx split, every dW split) the plan returns for the shape over PLAN_CUS, ascending"""
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    dx, dw = set(), set()
    for cus in PLAN_CUS:
        assert lib.y2_wide_head_train_plan(M, Kdim, Cout, cus, ctypes.byref(a), ctypes.byref(b)) == 0
        dx.add(a.value)
        dw.add(b.value)
    return sorted(dx), sorted(dw)


def reference(x, W, dy, s):
    """float64 on the operands as the kernels round them -> (dx, its bound, dW, its bound, db, its bound)"""
    M, Cout = dy.shape
    xh, Wh = x.astype(np.float16).astype(np.float64), W.astype(np.float16).astype(np.float64)
    dh = (np.float32(s) * dy).astype(np.float32).astype(np.float16).astype(np.float64)
    assert np.isfinite(dh).all()
    u = 2.0 ** -24
    dx = dh @ Wh.T / s
    dx_bound = 2.0 * Cout * u * (np.abs(dh) @ np.abs(Wh).T) / s + 1e-30
    dW = xh.T @ dh / s
    dW_bound = 2.0 * M * u * (np.abs(xh).T @ np.abs(dh)) / s + 1e-30
    db = dy.astype(np.float64).sum(0)
    db_bound = 2.0 * M * u * np.abs(dy.astype(np.float64)).sum(0) + 1e-30
    return dx, dx_bound, dW, dW_bound, db, db_bound


def guarded(n, seed):
    """(a NaN-filled float buffer of n elements with GUARD random words behind it, those words)"""
    import torch
    buf = torch.full((n + GUARD,), float("nan"), device="cuda")
    guard = dev(np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31, GUARD).astype(np.int32))
    buf[n:].view(torch.int32).copy_(guard)
    return buf, guard


def intact(buf, n, guard):
    import torch
    return torch.equal(buf[n:].view(torch.int32), guard)


def run_dx(lib, dyd, packed2, M, Kdim, Cout, s, split):
    import torch
    nws = lib.y2_wide_head_backward_input_workspace_bytes(M, Kdim, Cout, split)
    assert nws % 4 == 0
    out, g_out = guarded(M * Kdim, 1)
    ws, g_ws = guarded(nws // 4, 2)
    assert lib.y2_wide_head_backward_input(p(dyd), p(packed2), M, Kdim, Cout, s, p(out), p(ws), nws, split, None) == 0, \
        lib.y2_last_error()
    torch.cuda.synchronize()
    assert intact(out, M * Kdim, g_out) and intact(ws, nws // 4, g_ws)   # nothing behind dx or the workspace was written
    return host(out[:M * Kdim]).reshape(M, Kdim)


def run_dw(lib, xd, dyd, M, Kdim, Cout, s, split):
    import torch
    nws = lib.y2_wide_head_backward_filter_workspace_bytes(M, Kdim, Cout, split)
    dW, g_dW = guarded(Kdim * Cout, 3)
    db, g_db = guarded(Cout, 4)
    ws, g_ws = guarded(nws // 4, 5)
    assert lib.y2_wide_head_backward_filter(p(xd), p(dyd), M, Kdim, Cout, s, p(dW), p(db), p(ws), nws, split, None) == 0, \
        lib.y2_last_error()
    torch.cuda.synchronize()
    assert intact(dW, Kdim * Cout, g_dW) and intact(db, Cout, g_db) and intact(ws, nws // 4, g_ws)
    return host(dW[:Kdim * Cout]).reshape(Kdim, Cout), host(db[:Cout])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_products(M, Kdim, Cout, s=1.0, dy=None, tag=""):
    """both products and db at every split count of the plan (0: the entry's own choice on this device) -> (dW, db) of
    the entry's own choice"""
    lib = _lib()
    x, W, _b = K.gemm_operands(M, Kdim, Cout)
    dy = gradient(M, Cout) if dy is None else dy
    dx_ref, dx_bound, dW_ref, dW_bound, db_ref, db_bound = reference(x, W, dy, s)
    xd, Wd, dyd = dev(x), dev(W), dev(dy)
    import torch
    n2 = lib.y2_wide_head_packed2_bytes(Kdim, Cout)
    assert n2 == (Kdim + 127) // 128 * 128 * ((Cout + 63) // 64 * 64) * 2
    packed2 = torch.full((n2,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.y2_wide_head_pack2(p(Wd), Kdim, Cout, p(packed2), n2, None) == 0, lib.y2_last_error()
    dx_splits, dw_splits = plan_splits(lib, M, Kdim, Cout)
    worst = {"dx": 0.0, "dW": 0.0, "db": 0.0}
    for split in [0] + dx_splits:
        got = run_dx(lib, dyd, packed2, M, Kdim, Cout, s, split)
        assert np.isfinite(got).all(), split                              # the NaN prefill is fully overwritten
        assert same_bits(got, run_dx(lib, dyd, packed2, M, Kdim, Cout, s, split)), split
        ratio = (np.abs(got.astype(np.float64) - dx_ref) / dx_bound).max()
        worst["dx"] = max(worst["dx"], ratio)
        assert ratio <= 1.0, ("dx", split, ratio)
    keep = None
    for split in [0] + dw_splits:
        dW, db = run_dw(lib, xd, dyd, M, Kdim, Cout, s, split)
        assert np.isfinite(dW).all() and np.isfinite(db).all(), split
        if split in (0, dw_splits[-1]):
            again = run_dw(lib, xd, dyd, M, Kdim, Cout, s, split)
            assert same_bits(dW, again[0]) and same_bits(db, again[1]), split
        ratio = (np.abs(dW.astype(np.float64) - dW_ref) / dW_bound).max()
        rb = (np.abs(db.astype(np.float64) - db_ref) / db_bound).max()
        worst["dW"], worst["db"] = max(worst["dW"], ratio), max(worst["db"], rb)
        assert ratio <= 1.0 and rb <= 1.0, ("dW", split, ratio, rb)
        if split == 0:
            keep = (dW, db)
    print("wide head backward (%d, %d, %d)%s s = %g: dx splits %s, dW splits %s; largest |got - ref| / bound: dx %.4f, "
          "dW %.4f, db %.4f" % (M, Kdim, Cout, tag, s, dx_splits, dw_splits, worst["dx"], worst["dW"], worst["db"]))
    return keep


@pytest.mark.parametrize("M,Kdim,Cout", SHAPES)
def test_products_match_float64_on_the_rounded_operands(M, Kdim, Cout):
    check_products(M, Kdim, Cout)


def test_products_under_a_loss_scale_of_1024():
    check_products(147, 128, 2115, s=1024.0)


def test_the_tree_loss_sparsity_gives_exactly_zero_columns():
    """(147, 128, 2115) = 3 slots of 5 + 700: dy zero except for the 5 box columns of every slot -- and, in the first
    run, two full rows, as the rows of a truth are.  The second run leaves the two rows out, so every class column of dy
    is exactly zero: those columns of dW and those elements of db are zero (either sign)"""
    M, Kdim, Cout = 147, 128, 2115
    full = gradient(M, Cout, seed=1)
    box = np.zeros(Cout, bool)
    for slot in range(3):
        box[slot * 705:slot * 705 + 5] = True
    dy = np.where(box[None, :], full, np.float32(0))
    rows = dy.copy()
    rows[7], rows[100] = full[7], full[100]
    check_products(M, Kdim, Cout, dy=rows, tag=" sparse + two rows")
    dW, db = check_products(M, Kdim, Cout, dy=dy, tag=" sparse")
    assert not dW[:, ~box].any() and not db[~box].any()
    assert dW[:, box].all() and db[box].all()


class _Scaler:
    """what WideHeadSGD reads of a LossScaler: its control block"""

    def __init__(self, lr_t=0.0):
        self.ctrl = dev(np.zeros(8, np.int32))
        self.set(0, lr_t)

    def set(self, found_inf, lr_t):
        c = np.zeros(8, np.int32)
        c[0] = found_inf
        c[4] = np.float32(lr_t).view(np.int32)
        self.ctrl.copy_(dev(c))


def _operator(Kdim, Cout, seed=11):
    from tensorflow_yolo2_amd import engine as E
    _x, W, b = K.gemm_operands(3, Kdim, Cout)
    wide = E.WideHead(Kdim, Cout)
    wide.load(W, b)
    return wide, W, b


def _state(wide, opt):
    return [host(t) for t in (wide.W, wide.b, opt.accum, wide.packed, wide.packed2)]


SOLVER = dict(learning_rate=0.01, policy="constant", burn_in=0, steps=(), scales=())


def test_an_overflowed_operand_sets_the_flag_and_the_step_moves_nothing():
    """s dy above 65,504 in one element: f16(s dy) is inf, dW holds inf (or NaN) in that column; the scan is y2_range_check
    over dW and db at fp32's maximum"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    M, Kdim, Cout = 40, 96, 300
    wide, _W, _b = _operator(Kdim, Cout)
    x = dev(K.gemm_operands(M, Kdim, Cout)[0])
    dy = gradient(M, Cout)
    scaler = _Scaler(lr_t=0.01)
    opt = E.WideHeadSGD(wide, S.Solver(**SOLVER), scaler)
    opt.accum.copy_(dev(gradient(1, Kdim * Cout + Cout, seed=3)[0]))
    wide.backward(x, dev(dy), 1024.0)
    opt.scan()
    torch.cuda.synchronize()
    assert host(scaler.ctrl)[0] == 0 and torch.isfinite(wide.dW).all()   # a clean gradient leaves the flag alone
    dy[17, 123] = 100.0                                                   # 1024 x 100 = 102,400 > 65,504
    wide.backward(x, dev(dy), 1024.0)
    assert not torch.isfinite(wide.dW[0, 0, :, 123]).any() and torch.isfinite(wide.db).all()
    before = _state(wide, opt)
    opt.scan()
    opt.step(grad_mult=1.0, joint="next")
    torch.cuda.synchronize()
    assert host(scaler.ctrl)[0] == 1
    for a, b in zip(before, _state(wide, opt)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    with pytest.raises(ValueError, match="next"):
        opt.step(joint="first")


def test_two_solver_steps_follow_the_specification_and_keep_both_images_current():
    """random W, b, accum and gradients, grad_mult 0.5, decay on: utils/solver.py sgd_step within 1 ulp (its fma goes
    through float64: tests/test_gpu_sgd_solver.py), b with decay off; both images bit-equal to a fresh pack of the new W,
    padding zero.  The third step reads its rate from a control block"""
    import torch
    from tensorflow_yolo2_amd import engine as E
    Kdim, Cout = 96, 300
    lib = _lib()
    wide, _W, _b = _operator(Kdim, Cout)
    sv = S.Solver(**SOLVER)
    assert sv.decay == 0.0005 and sv.momentum == 0.9
    opt = E.WideHeadSGD(wide, sv)
    rng = np.random.default_rng(5)
    opt.accum.copy_(dev((rng.standard_normal(Kdim * Cout + Cout) * 1e-2).astype(np.float32)))
    wide.dW, wide.db = torch.empty_like(wide.W), torch.empty_like(wide.b)
    scaler = _Scaler()
    for t in (1, 2, 3):
        gW = (rng.standard_normal((1, 1, Kdim, Cout)) * 1e-2).astype(np.float32)
        gb = (rng.standard_normal(Cout) * 1e-2).astype(np.float32)
        wide.dW.copy_(dev(gW))
        wide.db.copy_(dev(gb))
        W0, b0, acc0 = host(wide.W).ravel(), host(wide.b), host(opt.accum)
        rate = S.current_rate(sv, t)
        if t == 3:
            rate = np.float32(0.003)
            scaler.set(0, rate)
            opt.scaler = scaler
        opt.step(grad_mult=0.5)
        torch.cuda.synchronize()
        half = np.float32(0.5)
        want_W, want_aW = S.sgd_step(W0, acc0[:Kdim * Cout], (gW.ravel() * half).astype(np.float32), rate, sv.momentum,
                                     sv.decay, True)
        want_b, want_ab = S.sgd_step(b0, acc0[Kdim * Cout:], (gb * half).astype(np.float32), rate, sv.momentum, sv.decay,
                                     False)
        acc = host(opt.accum)
        dW_, db_ = ulps(host(wide.W).ravel(), want_W).max(), ulps(host(wide.b), want_b).max()
        daW, dab = ulps(acc[:Kdim * Cout], want_aW).max(), ulps(acc[Kdim * Cout:], want_ab).max()
        print("wide head step %d: W within %d ulp, b %d, accum %d and %d" % (t, dW_, db_, daW, dab))
        assert max(dW_, db_, daW, dab) <= 1, t
        assert not np.array_equal(host(wide.W).ravel(), W0) and not np.array_equal(host(wide.b), b0)
        # decay reaches W and not b: the specification with the masks exchanged is far away
        far_W = S.sgd_step(W0, acc0[:Kdim * Cout], (gW.ravel() * half).astype(np.float32), rate, sv.momentum, sv.decay, False)
        assert ulps(acc[:Kdim * Cout], far_W[1]).max() > 100
        Wd = wide.W.view(Kdim, Cout)
        assert np.array_equal(host(wide.packed), host(K.packed_image(lib, Wd, Kdim, Cout)))
        fresh = torch.full((wide.packed2.numel(),), 0xAB, dtype=torch.uint8, device="cuda")
        assert lib.y2_wide_head_pack2(p(Wd), Kdim, Cout, p(fresh), fresh.numel(), None) == 0
        assert np.array_equal(host(wide.packed2), host(fresh))
        image2 = host(wide.packed2).view(np.float16).reshape(128, 320)
        assert np.array_equal(image2[:Kdim, :Cout].view(np.uint16), host(Wd).astype(np.float16).view(np.uint16))
        assert not image2[Kdim:].view(np.uint16).any() and not image2[:, Cout:].view(np.uint16).any()
        image = host(wide.packed).view(np.float16).reshape(512, 128)
        assert not image[Cout:].view(np.uint16).any() and not image[:, Kdim:].view(np.uint16).any()
    state = opt.export_state()
    assert state["t"] == 3 and state["accum"].shape == (Kdim * Cout + Cout,)
    other = E.WideHeadSGD(wide, sv)
    other.load_state(state)
    assert other.t == 3 and np.array_equal(host(other.accum), state["accum"])
    with pytest.raises(ValueError, match="Adam"):
        E.WideHeadSGD(wide, None)


def test_training_entries_reject_bad_arguments():
    import torch
    lib = _lib()
    M, Kdim, Cout = 70, 64, 200                                          # two reduction steps each way: a split of 2 exists
    x, Wt, b = K.gemm_operands(M, Kdim, Cout)
    xd, Wd, bd, dyd = dev(x), dev(Wt), dev(b), dev(gradient(M, Cout))
    n1, n2 = lib.y2_wide_head_packed_bytes(Kdim, Cout), lib.y2_wide_head_packed2_bytes(Kdim, Cout)
    packed = torch.full((n1 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    packed2 = torch.full((n2 + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    dx = torch.full((M * Kdim,), 7.0, device="cuda")
    dW = torch.full((Kdim * Cout,), 7.0, device="cuda")
    db = torch.full((Cout,), 7.0, device="cuda")
    accum = torch.full((Kdim * Cout + Cout,), 7.0, device="cuda")
    ws = torch.full((4 * M * Kdim + 4 * Kdim * Cout + 16,), 7.0, device="cuda")
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    f = ctypes.c_float
    tables = {
        "y2_wide_head_pack2": (("W", p(Wd)), ("K", Kdim), ("Cout", Cout), ("packed2", p(packed2)), ("bytes", n2), ("stream", None)),
        "y2_wide_head_backward_input": (("dy", p(dyd)), ("packed2", p(packed2)), ("M", M), ("K", Kdim), ("Cout", Cout),
                                        ("s", f(1.0)), ("dx", p(dx)), ("ws", p(ws)), ("ws_bytes", ws.numel() * 4),
                                        ("split", 0), ("stream", None)),
        "y2_wide_head_backward_filter": (("x", p(xd)), ("dy", p(dyd)), ("M", M), ("K", Kdim), ("Cout", Cout), ("s", f(1.0)),
                                         ("dW", p(dW)), ("db", p(db)), ("ws", p(ws)), ("ws_bytes", ws.numel() * 4),
                                         ("split", 0), ("stream", None)),
        "y2_wide_head_sgd_step": (("W", p(Wd)), ("b", p(bd)), ("accum", p(accum)), ("dW", p(dW)), ("db", p(db)), ("K", Kdim),
                                  ("Cout", Cout), ("packed", p(packed)), ("bytes", n1), ("packed2", p(packed2)),
                                  ("bytes2", n2), ("ctrl", None), ("lr", f(0.01)), ("momentum", f(0.9)), ("decay", f(0.0005)),
                                  ("grad_mult", f(1.0)), ("stream", None)),
    }
    shared = ((dict(K=0), b"K = 0"), (dict(K=48), b"multiple of 32"), (dict(K=4128), b"at most 4096"),
              (dict(Cout=0), b"Cout = 0"), (dict(Cout=65536 * 16 + 1), b"Cout = 1048577"), (dict(packed2=None), b"null"),
              (dict(packed2=off(packed2, 8)), b"16-byte aligned"))
    products = ((dict(M=0), b"M = 0"), (dict(M=-3), b"at least 1"), (dict(dy=None), b"null"), (dict(s=f(0.0)), b"grad_scale"),
                (dict(s=f(-2.0)), b"grad_scale"), (dict(s=f(float("inf"))), b"grad_scale"), (dict(s=f(float("nan"))), b"grad_scale"),
                (dict(split=-1), b"split = -1"), (dict(split=2, ws=None), b"workspace_bytes"),
                (dict(split=2, ws_bytes=15), b"workspace_bytes"), (dict(split=2, ws=off(ws, 4)), b"workspace is not 16-byte"))
    more = {"y2_wide_head_pack2": ((dict(W=None), b"null"), (dict(bytes=n2 - 1), b"packed2_bytes")),
            "y2_wide_head_backward_input": products + ((dict(dx=None), b"null"), (dict(dy=off(dyd, 2)), b"4-byte aligned")),
            "y2_wide_head_backward_filter": tuple(r for r in products if "packed2" not in r[0]) +
            ((dict(x=None), b"null"), (dict(dW=None), b"null"), (dict(db=None), b"null"), (dict(x=off(xd, 4)), b"16-byte aligned")),
            "y2_wide_head_sgd_step": ((dict(W=None), b"null"), (dict(b=None), b"null"), (dict(accum=None), b"null"),
                                      (dict(dW=None), b"null"), (dict(db=None), b"null"), (dict(packed=None), b"null"),
                                      (dict(packed=off(packed, 8)), b"16-byte aligned"), (dict(bytes=n1 - 1), b"packed_bytes"),
                                      (dict(bytes2=n2 - 1), b"packed2_bytes"), (dict(lr=f(-1.0)), b"lr = -1"),
                                      (dict(lr=f(float("nan"))), b"lr = nan"), (dict(momentum=f(1.0)), b"momentum = 1"),
                                      (dict(decay=f(-0.5)), b"decay = -0.5"))}
    for name, table in tables.items():
        call = lambda **kw: getattr(lib, name)(*[kw.get(k, v) for k, v in table])
        rows = [r for r in shared if set(r[0]) <= {k for k, _v in table}] + list(more[name])
        for kw, word in rows:
            assert call(**kw) == -1, (name, kw)                           # Y2_ERR_ARG
            err = lib.y2_last_error()
            assert name.encode() in err and word in err, (name, kw, err)
    a, c = ctypes.c_int(0), ctypes.c_int(0)
    for bad, word in (((0, 64, 10, 256), b"M = 0"), ((5, 48, 10, 256), b"multiple of 32"), ((5, 64, 0, 256), b"Cout = 0"),
                      ((5, 64, 10, 0), b"cus = 0")):
        assert lib.y2_wide_head_train_plan(*bad, ctypes.byref(a), ctypes.byref(c)) == -1
        assert b"y2_wide_head_train_plan" in lib.y2_last_error() and word in lib.y2_last_error()
    assert lib.y2_wide_head_train_plan(5, 64, 10, 256, None, ctypes.byref(c)) == -1 and b"null" in lib.y2_last_error()
    for bad in ((0, 10), (48, 10), (4128, 10), (64, 0), (64, 65536 * 16 + 1)):
        assert lib.y2_wide_head_packed2_bytes(*bad) == 0, bad
        assert lib.y2_wide_head_backward_input_workspace_bytes(5, bad[0], bad[1], 2) == 0
        assert lib.y2_wide_head_backward_filter_workspace_bytes(5, bad[0], bad[1], 2) == 0
    torch.cuda.synchronize()
    for t in (dx, dW, db, accum, ws):
        assert (t == 7.0).all()                                           # nothing was launched
    assert (packed == 0xAB).all() and (packed2 == 0xAB).all()
    assert np.array_equal(host(Wd), Wt) and np.array_equal(host(bd), b)
    for name, table in tables.items():
        assert getattr(lib, name)(*[v for _k, v in table]) == 0, lib.y2_last_error()
    torch.cuda.synchronize()
    assert not (dx == 7.0).any() and not (dW == 7.0).any() and not (db == 7.0).any() and not (accum == 7.0).any()
    assert (packed[n1:] == 0xAB).all() and (packed2[n2:] == 0xAB).all() and not (packed2[:n2] == 0xAB).all()


def _truths(n):
    """a box list with two truths in one cell of image 0 and no truth in image 1 (classes: nodes of the 700-node tree)"""
    truth = np.zeros((n, 30, 5), np.float32)
    truth[0, 0] = (1.3 * 32, 1.6 * 32, 45.0, 58.0, 90)
    truth[0, 1] = (1.7 * 32, 1.4 * 32, 40.0, 36.0, 125)
    return dev(truth), dev(np.array([2] + [0] * (n - 1), np.int32))


def test_trainer_from_the_wide_cfg_steps_saves_and_runs_in_a_detector(tmp_path):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    n = 2
    cfg = K.write_wide_model_files(tmp_path)
    sv = S.Solver(**dict(SOLVER, learning_rate=0.001))
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, batch=n, image_size=160, dtype="f16", wide_head=True, solver=sv, seed=3)
    assert tr.wide is not None and (tr.wide.K, tr.wide.Cout) == (128, 2115) and tr.tree.n == 700 and tr.B == 3
    assert isinstance(tr.wide_opt, E.WideHeadSGD) and tr.wide_opt.scaler is tr.opts[0].scaler
    src = K.random_weights_file(str(tmp_path / "wide.weights"), tr.cfg.file_layers, seed=21)
    assert net_utils.load_darknet_weights(tr, src) == 1234
    truth, ntruth = _truths(n)
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8))
    W0, b0 = host(tr.wide.W), host(tr.wide.b)
    scale = tr.opts[0].scaler.scale
    loss = tr.step(x, truth=truth, ntruth=ntruth)
    torch.cuda.synchronize()
    assert np.isfinite(host(loss)).all() and tr.opts[0].scaler.state() == (0, 1, 0)
    # the wide layer's gradients are WideHead.backward of the kept operands, and its dx is what the head stack was given
    assert tuple(tr.last_wide_x.shape) == (n, 5, 5, 128) and tr.last_dnet.numel() == n * 25 * 2115
    alone = E.WideHead(128, 2115)
    alone.load(W0, b0)
    dx = alone.backward(tr.last_wide_x, tr.last_dnet, scale)
    torch.cuda.synchronize()
    assert same_bits(host(alone.dW), host(tr.wide.dW)) and same_bits(host(alone.db), host(tr.wide.db))
    assert same_bits(host(dx), host(tr.last_wide_dx)) and host(dx).any() and host(tr.wide.dW).any()
    grads = tr.wide.export_grads()
    assert grads["W"].shape == (1, 1, 128, 2115) and same_bits(grads["b"], host(tr.wide.db))
    # the head stack's last layer is an ordinary layer here: its gamma trains
    head = tr.nets[-1]
    assert host(head.layer_views(head.num_layers - 1, grads=True)["gamma"]).any()
    # the update of W and b
    rate = S.current_rate(sv, 1)
    zero = np.zeros(W0.size, np.float32)
    want_W, _acc = S.sgd_step(W0.ravel(), zero, host(tr.wide.dW).ravel(), rate, sv.momentum, sv.decay, True)
    want_b, _acc = S.sgd_step(b0, zero[:b0.size], host(tr.wide.db), rate, sv.momentum, sv.decay, False)
    assert ulps(host(tr.wide.W).ravel(), want_W).max() <= 1 and ulps(host(tr.wide.b), want_b).max() <= 1
    assert not np.array_equal(host(tr.wide.W), W0)
    # another input size
    x192 = dev(np.random.default_rng(9).integers(0, 256, (n, 192, 192, 3), dtype=np.uint8))
    loss = tr.step(x192, truth=truth, ntruth=ntruth)
    torch.cuda.synchronize()
    assert np.isfinite(host(loss)).all() and tr.opts[0].scaler.state() == (0, 2, 0)
    # written, read by a detector: the same raw head, bit for bit
    out = str(tmp_path / "trained.weights")
    net_utils.save_darknet_weights(tr, out, 1234 + 2 * n)
    det = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16", wide_head=True)
    assert net_utils.load_darknet_weights(det, out) == 1234 + 2 * n
    for net in tr.networks(160):
        net.params_changed()                                              # the 192 contexts moved the shared parameters
    want, _fine = tr.forward(x, training=False)
    got = det.forward(x)
    torch.cuda.synchronize()
    assert same_bits(host(got), host(want))


def test_detector_train_writes_and_resumes_the_wide_model(tmp_path, golden_dir, capsys):
    """darknet/detector.py train (pascal_train_yolov2's main) on the wide cfg: the file loads with the wide head by
    itself, the snapshot is a `.weights` file of the cfg's float count, and a second run resumes from it"""
    import os
    from test_gpu_device_darknet import make_list
    from tensorflow_yolo2_amd.darknet import detector
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    root = str(tmp_path)
    cfg = K.write_wide_model_files(tmp_path)
    lst = make_list(root, golden_dir)
    data = os.path.join(root, "wide.data")
    with open(data, "w") as f:
        f.write("classes = 700\ntrain = %s\nbackup = %s\n" % (lst, os.path.join(root, "backup")))
    first = detector.main(["train", data, cfg, "--iters", "2", "--single-scale"])
    out = capsys.readouterr().out
    assert "topology tiny, 700 classes, 3 anchors, size 160, batch 2, multi-scale off" in out
    tr = first["trainer"]
    assert tr.wide is not None and (tr.wide.K, tr.wide.Cout) == (128, 2115) and tr.wide_opt is not None
    assert np.isfinite(np.array(first["losses"])).all() and len(first["losses"]) == 2
    snap = os.path.join(root, "backup", "train_iter_2.weights")
    assert os.path.exists(snap) and DW.read(snap)[3] == 4 and DW.read(snap)[4].size == tr.cfg.floats
    W2 = host(tr.wide.W)
    second = detector.main(["train", data, cfg, "--iters", "1", "--single-scale"])
    assert "Restorining model snapshots from " + snap in capsys.readouterr().out
    assert second["first_iter"] == 3 and second["last_iter"] == 3 and np.isfinite(np.array(second["losses"])).all()
    assert second["trainer"].wide_opt.t == 3 and not np.array_equal(host(second["trainer"].wide.W), W2)
    assert os.path.exists(os.path.join(root, "backup", "train_iter_3.weights"))


def test_what_a_wide_trainer_refuses(tmp_path):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    cfg = K.write_wide_model_files(tmp_path)
    for dtype in ("f32", "bf16", "f16x2", "f16x2f", "fp8"):
        with pytest.raises(ValueError) as e:
            yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, batch=2, image_size=160, dtype=dtype, wide_head=True)
        assert "dtype %r" % dtype in str(e.value) and "'f16' only" in str(e.value)
    topo, record = yolov2._cfg_topology(cfg, "f16", True, training=True)
    with pytest.raises(ValueError, match="solver"):
        yolov2.YOLOv2DarknetTrainer(2, 160, num_class=record.classes, anchors=record.anchors, dtype="f16",
                                    _cfg=(topo, record), tree=yolov2.load_cfg_tree(record))
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, batch=2, image_size=160, dtype="f16", wide_head=True)
    x = dev(np.zeros((2, 160, 160, 3), np.uint8))
    with pytest.raises(ValueError, match="label grid with a word tree"):
        tr.step(x, labels=dev(np.zeros((2, 5, 5, 705), np.float32)))
