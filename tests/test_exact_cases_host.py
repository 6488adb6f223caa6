"""Host test of what tests/test_gpu_exact_forms.py relies on: the case table of tests/_exact_cases.py is well formed,
its seeds are fixed and distinct, every case adds a form key (or states why it is there), and the float64 reference of
every case -- computed here on the CPU by the same function the device test calls -- stays inside the magnitudes at which
f16, bf16 and fp32 hold every integer exactly."""
import numpy as np
import pytest
import torch

import _exact_cases as X


def test_table_is_well_formed():
    assert len(set(X.CASE_IDS)) == len(X.CASES)
    seeds = [c[7] for c in X.CASES]
    assert seeds == list(range(1000, 1000 + len(X.CASES))), "seeds are fixed: 1000 + the case's position"
    for name, N, H, W, cin, cout, k, seed, fwd, dgrad, wgrad in X.CASES:
        assert name == "%dx%d_%dto%d_n%d_%dx%d" % (k, k, cin, cout, N, H, W)
        assert k in (1, 3) and min(N, H, W, cin, cout) >= 1
        assert fwd[0] in range(7) and dgrad[0] in range(7) and fwd[2] in (0, 1) and dgrad[2] in (0, 1)
        # the K-split kinds and the K-split flag say the same thing
        for form in (fwd, dgrad):
            assert (form[0] in (X.CK_HALOQ_KS, X.CK_IGEMM_KS)) == bool(form[2]), name
        assert wgrad[0] in (X.WK_TAP, X.WK_NINE, X.WK_RING) and wgrad[2] in (0, 1)
        # one partial per element is stored directly; more go through the slab, or through atomics when they outgrow it
        assert (wgrad[3] == X.WS_DIRECT) == (wgrad[2] == 0), name
        if wgrad[3] == X.WS_ATOMIC:
            cin_p = 32 if cin <= 32 else 64 if cin <= 64 else (cin + 127) // 128 * 128
            assert 2 * k * k * cin_p * cout > 1024 * 18432, name
        # 1x1 layers take the per-tap kernel; 3x3 ones only where the rows are too long for the nine-tap families
        assert wgrad[0] == X.WK_TAP if k == 1 else (wgrad[0] != X.WK_TAP or W > 380), name
    for name in X.ATOMIC_CASES:
        assert X.CASES[X.CASE_IDS.index(name)][10][2] == 1, "the atomics route needs more than one partial"
    assert {X.CASES[X.CASE_IDS.index(n)][10][0] for n in X.ATOMIC_CASES} == {X.WK_TAP, X.WK_NINE, X.WK_RING}


def test_every_case_adds_a_form_key_or_says_why():
    seen = set()
    for case in X.CASES:
        keys = set(X.case_keys(case, "f16"))
        if keys <= seen:
            assert case[0] in X.DUPLICATE_REASONS, "%s pins no form key of its own and states no reason" % case[0]
        seen |= keys
    assert set(X.DUPLICATE_REASONS) <= set(X.CASE_IDS)
    # f16 and bf16 take identical plans: the keys differ in the launch dtype alone
    for case in X.CASES:
        for a, b in zip(X.case_keys(case, "f16"), X.case_keys(case, "bf16")):
            assert a[1] == 1 and b[1] == 2 and a[:1] + a[2:] == b[:1] + b[2:]


def test_data_is_small_integers_at_the_stated_density():
    case = X.CASES[X.CASE_IDS.index("3x3_96to125_n256_14x14")]
    x, w, b, dy = X.case_data(case)
    x2 = X.case_data(case)[0]
    assert np.array_equal(x, x2), "the data is a function of the seed alone"
    for a in (x, w, dy):
        assert a.dtype == np.float32 and set(np.unique(a)) == {-1.0, 0.0, 1.0}
    assert set(np.unique(b)) <= {-1.0, 0.0, 1.0}
    Kf, Kd = 9 * 96, 9 * 125
    assert abs((x != 0).mean() - X.density(Kf)) < 0.01 and abs((dy != 0).mean() - X.density(Kd)) < 0.01
    assert abs((w != 0).mean() - X.density(max(Kf, Kd))) < 0.01
    assert X.density(288) == 0.5 and abs(X.density(9216) - np.sqrt(1000 / 9216)) < 1e-12


@pytest.mark.parametrize("name", X.CASE_IDS)
def test_reference_magnitudes_keep_every_type_exact(name):
    case = X.CASES[X.CASE_IDS.index(name)]
    x, w, b, dy = (torch.as_tensor(a) for a in X.case_data(case))
    y, dx, dw = X.reference(x, w, b, dy)
    my, mdx, mdw = X.check_magnitudes(name, y, dx, dw)
    assert my <= X.STORE_MAX["bf16"] <= X.STORE_MAX["f16"] and mdx <= X.STORE_MAX["bf16"] and mdw < 2 ** 24
    # integers, and nothing degenerate: a zero tensor would pass any kernel
    for t in (y, dx, dw):
        assert torch.equal(t, t.round()) and float(t.abs().max()) >= 1


@pytest.mark.parametrize("name", X.NET_CASE_IDS)
def test_network_case_outputs_stay_exact_in_bf16(name):
    """layer 0 of every network case: integer data, a conv output (bias and its offsets included) within bf16's integers"""
    import torch.nn.functional as F
    case = X.NET_CASES[X.NET_CASE_IDS.index(name)]
    x, w, b = (torch.as_tensor(a) for a in X.net_case_data(case))
    assert all(torch.equal(t, t.round()) for t in (x, w, b)) and float(b.abs().max()) > 1, "some channels carry an offset"
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(3, 2, 0, 1), b.double(), padding=w.shape[0] // 2)
    assert 1 <= float(y.abs().max()) <= X.STORE_MAX["bf16"], (name, float(y.abs().max()))
    assert len(set(c[6] for c in X.NET_CASES)) == len(X.NET_CASES)
    (k0, cin, c1, pool), (k1, c2) = case[4], case[5]
    assert cin % 32 == 0 and (cin <= 128 or cin % 128 == 0) and (c1 in (32, 64) or c1 % 128 == 0), "channels both passes take"
    assert not pool or (case[2] % 2 == 0 and case[3] % 2 == 0)


def test_reference_is_the_convolution_and_its_gradients():
    """the per-tap float64 reference against torch's own conv2d and autograd, at a 3x3 and a 1x1 case"""
    import torch.nn.functional as F
    for name in ("3x3_32to125_n8_7x7", "1x1_96to64_n8_7x7"):
        case = X.CASES[X.CASE_IDS.index(name)]
        x, w, b, dy = (torch.as_tensor(a) for a in X.case_data(case))
        y, dx, dw = X.reference(x, w, b, dy)
        xt = x.double().permute(0, 3, 1, 2).requires_grad_(True)
        wt = w.double().permute(3, 2, 0, 1).requires_grad_(True)
        yt = F.conv2d(xt, wt, b.double(), padding=w.shape[0] // 2)
        yt.backward(dy.double().permute(0, 3, 1, 2))
        assert torch.equal(y, yt.permute(0, 2, 3, 1))
        assert torch.equal(dx, xt.grad.permute(0, 2, 3, 1))
        assert torch.equal(dw, wt.grad.permute(2, 3, 1, 0))


def test_mismatch_report_names_the_wrong_elements():
    ref = torch.zeros(2, 3, 4, 5, dtype=torch.float64)
    got = ref.clone()
    assert X.mismatch_report("y", got, ref, ("image", "row", "column", "channel")) == ""
    got[1, 2, 0, 3] = 7
    msg = X.mismatch_report("y", got, ref, ("image", "row", "column", "channel"))
    assert "1 of 120" in msg and "image 1, row 2, column 0, channel 3" in msg and "got 7 want 0" in msg
