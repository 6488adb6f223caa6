"""y2_score_views (csrc/score.hip) on the GPU against its float64 specification utils/score_views.score_views_ref: the
classes, ranks and counters by equality, the probabilities within a bound derived from the float32 operations, and the
same bits from a second call.

The bound, relative, with u = 2^-24 and dmax = max(max_v - x) over the case's logits:
    bound = (2 * dmax + C + V + 8) * u
2 * dmax * u covers one rounding of the subtraction x - max_v carried through exp (numerator and denominator), C * u a
worst-case ordered sum of C terms, the rest a 1-ulp expf, the division and the mean over the views.  Every seeded case
asserts first that the float64 scores of sorted positions 0 .. 8 lie at least 2 * bound apart (relative), so that the
order of the float32 scores is the reference's."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 4                                       # words after every output buffer
SEEDED = [(3, 10, 1000), (3, 2, 257), (2, 10, 63), (3, 5, 21), (1, 3, 5), (4, 2, 64), (2, 16, 256)]


def _ref(*a, **k):
    from tensorflow_yolo2_amd.utils.score_views import score_views_ref
    return score_views_ref(*a, **k)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call(x, labels, k, n_valid=None, hits=None, want=("prob", "rank", "hits")):
    """the C entry on x [n, V, C] float32 with guard words after every output -> dict of numpy outputs (the guards are
    checked here), 'rc' the return code"""
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    n, V, Cn = x.shape
    xd = torch.from_numpy(x.reshape(n * V, Cn).copy()).cuda()
    ld = torch.from_numpy(np.asarray(labels, np.int64).astype(np.int32)).cuda() if labels is not None else None
    sizes = {"top_idx": (n * k, torch.int32), "top_val": (n * k, torch.float32), "prob": (n * Cn, torch.float32),
             "rank": (n, torch.int32), "hits": (4, torch.int32)}
    buf = {}
    for name, (size, dtype) in sizes.items():
        if name in ("top_idx", "top_val") or (name in want and (labels is not None or name == "prob")):
            buf[name] = torch.full((size + GUARD,), 7777, dtype=dtype, device="cuda")
    if "hits" in buf:
        buf["hits"][:4] = torch.from_numpy(np.asarray(hits if hits is not None else [0, 0, 0, 0], np.int32)).cuda()
    rc = lib.y2_score_views(_ptr(xd), _ptr(ld), n, V, Cn, k, n if n_valid is None else n_valid, _ptr(buf.get("prob")),
                            _ptr(buf["top_idx"]), _ptr(buf["top_val"]), _ptr(buf.get("rank")), _ptr(buf.get("hits")),
                            None)
    torch.cuda.synchronize()
    out = {"rc": rc}
    for name, t in buf.items():
        h = t.cpu().numpy()
        assert (h[-GUARD:] == 7777).all(), (name, h[-GUARD:])
        out[name] = h[:-GUARD]
    out["top_idx"], out["top_val"] = out["top_idx"].reshape(n, k), out["top_val"].reshape(n, k)
    if "prob" in out:
        out["prob"] = out["prob"].reshape(n, Cn)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def _seeded(n, V, Cn):
    """(x float32, labels, k, bound, the reference's outputs): computed once per shape and shared, never modified"""
    x = np.float32(3 * np.random.default_rng([0, V, Cn]).standard_normal((n, V, Cn)))
    x.setflags(write=False)
    k = 8 if Cn == 5 else 5
    x64 = x.astype(np.float64)
    dmax = float((x64.max(axis=2, keepdims=True) - x64).max())
    bound = (2 * dmax + Cn + V + 8) * U
    _, _, _, _, prob = _ref(x, views=V, k=k)
    order = np.argsort(-prob, axis=1, kind="stable")
    positions = [0, k - 1, k]
    labels = np.array([order[b, min(positions[b % 3], Cn - 1)] for b in range(n)], np.int64)
    return x, labels, k, bound, _ref(x, labels, views=V, k=k), prob


@pytest.mark.parametrize("shape", SEEDED)
def test_seeded_cases_equal_the_specification(shape):
    n, V, Cn = shape
    x, labels, k, bound, (ridx, rval, rrank, rhits, rprob), _ = _seeded(*shape)
    # the precondition: the scores that decide the outputs are further apart than twice the bound
    s = -np.sort(-rprob, axis=1)[:, :9]
    gap = ((s[:, :-1] - s[:, 1:]) / s[:, :-1]).min()
    print("shape %r: dmax bound %.3g, smallest relative gap of positions 0..8 %.3g" % (shape, bound, gap))
    assert gap >= 2 * bound, (shape, gap, bound)
    got = _call(x, labels, k)
    assert got["rc"] == 0
    err_val = np.abs(got["top_val"] - rval)[rval > 0] / rval[rval > 0]
    err_prob = np.abs(got["prob"] - rprob) / rprob
    print("  top_val error %.3g, prob error %.3g (relative, max)" % (err_val.max(), err_prob.max()))
    assert (got["top_idx"] == ridx).all(), (got["top_idx"], ridx)
    assert (got["rank"] == rrank).all() and (got["hits"] == rhits).all(), (got["rank"], rrank, got["hits"], rhits)
    assert set(rrank.tolist()) <= {0, k - 1, k} and rhits[0] == n
    assert err_val.max() <= bound and err_prob.max() <= bound, (err_val.max(), err_prob.max(), bound)
    own = np.argsort(-got["prob"], axis=1, kind="stable")       # views > 1: the order is that of the kernel's own p
    assert (got["top_idx"][:, :min(k, Cn)] == own[:, :k]).all()
    assert (got["rank"] == [own[b].tolist().index(labels[b]) for b in range(n)]).all()
    assert (got["top_val"][ridx < 0] == 0).all() and ((ridx < 0).sum() == n * max(k - Cn, 0))
    # a second call: the same bits everywhere; the counters accumulate
    again = _call(x, labels, k, hits=got["hits"])
    for name in ("top_idx", "top_val", "prob", "rank"):
        assert (_bits(again[name]) == _bits(got[name])).all(), name
    assert (again["hits"] == 2 * rhits).all()


def test_n_valid_masks_the_counters_alone_and_null_outputs_are_left_out():
    x, labels, k, bound, ref, _ = _seeded(3, 5, 21)
    full = _call(x, labels, k)
    part = _call(x, labels, k, n_valid=1, hits=[10, 5, 7, 1])
    want = _ref(x, labels, views=5, k=k, n_valid=1, hits=[10, 5, 7, 1])[3]
    assert (part["hits"] == want).all() and part["hits"][0] == 11
    for name in ("top_idx", "top_val", "prob", "rank"):
        assert (_bits(part[name]) == _bits(full[name])).all(), name
    none = _call(x, labels, k, n_valid=0)
    assert (none["hits"] == 0).all() and (none["rank"] == full["rank"]).all()
    bare = _call(x, None, k, want=())                           # no labels, no prob: the classes alone
    assert sorted(bare) == ["rc", "top_idx", "top_val"] and bare["rc"] == 0
    assert (bare["top_idx"] == full["top_idx"]).all() and (_bits(bare["top_val"]) == _bits(full["top_val"])).all()


def test_one_view_orders_by_the_logits():
    """exact duplicates, a pair one ulp apart, a row of equal logits, labels at index 0 and C - 1: the order is the
    logits' whatever their probabilities round to -- no precondition"""
    n, Cn, k = 5, 1000, 5
    x = np.float32(np.random.default_rng(11).standard_normal((n, 1, Cn)))
    top = np.float32(x.max() + 1)
    x[0, 0, 17] = x[0, 0, 400] = top                            # duplicates: 17 before 400
    x[1, 0, 3], x[1, 0, 900] = top, np.nextafter(top, np.float32(np.inf))   # one ulp: 900 before 3
    x[4, 0, :] = np.float32(0.25)                               # every class equal: the index order
    labels = [400, 3, 0, Cn - 1, 7]
    ridx, rval, rrank, rhits, rprob = _ref(x, labels, views=1, k=k)
    assert ridx[0, :2].tolist() == [17, 400] and ridx[1, :2].tolist() == [900, 3] and ridx[4].tolist() == [0, 1, 2, 3, 4]
    assert rrank[:2].tolist() == [1, 1] and rrank[4] == 7
    got = _call(x, labels, k)
    assert (got["top_idx"] == ridx).all() and (got["rank"] == rrank).all() and (got["hits"] == rhits).all()
    x64 = x.astype(np.float64)
    bound = (2 * float((x64.max(axis=2, keepdims=True) - x64).max()) + Cn + 1 + 8) * U
    assert (np.abs(got["prob"] - rprob) / rprob).max() <= bound
    assert (np.abs(got["top_val"] - rval) / rval).max() <= bound
    # a single class
    one = np.array([[[0.3]], [[-2.0]]], np.float32)
    got = _call(one, [0, 0], k)
    assert got["top_idx"].tolist() == [[0, -1, -1, -1, -1]] * 2 and got["top_val"].tolist() == [[1, 0, 0, 0, 0]] * 2
    assert got["rank"].tolist() == [0, 0] and got["hits"].tolist() == [2, 2, 2, 0] and got["prob"].tolist() == [[1], [1]]


def test_top_1_share_is_the_accuracy_kernel_s():
    import torch
    from tensorflow_yolo2_amd import engine as E
    n, Cn = 64, 1000
    x = np.float32(np.random.default_rng(12).standard_normal((n, Cn)))
    labels = np.random.default_rng(13).integers(0, Cn, n)
    labels[::3] = x[::3].argmax(axis=1)
    xd, ld = torch.from_numpy(x).cuda(), torch.from_numpy(labels.astype(np.int32)).cuda()
    top_idx, top_val, rank, hits, prob = E.score_views(xd, ld, views=1, k=5)
    assert prob is None and top_idx.shape == (n, 5) and rank.shape == (n,)
    acc = float(E.accuracy(xd, ld))
    h = hits.cpu().numpy()
    want = int((x.argmax(axis=1) == labels).sum())
    assert want >= 22 and h[0] == n and h[1] == want and h[1] / 64.0 == acc and h[3] == 0
    # caller-supplied tensors are the ones written; labels are optional
    mine = torch.zeros(4, dtype=torch.int32, device="cuda")
    ranks = torch.full((n + 1,), -9, dtype=torch.int32, device="cuda")
    out = E.score_views(xd, ld, views=1, k=5, hits=mine, rank=ranks[:n], want_prob=True)
    out = E.score_views(xd, ld, views=1, k=5, hits=mine, rank=ranks[:n], prob=out[4], n_valid=10)
    assert out[3] is mine and mine.cpu().numpy()[0] == n + 10 and ranks[n].item() == -9
    assert torch.equal(ranks[:n], rank) and out[4].shape == (n, Cn)
    bare = E.score_views(xd, views=2, k=3)
    assert bare[0].shape == (n // 2, 3) and bare[2] is None and bare[3] is None and bare[4] is None
    with pytest.raises(ValueError, match="multiple of views"):
        E.score_views(xd, views=3)


def test_identical_class_columns_come_out_bit_equal_and_in_index_order():
    n, V, Cn, k = 2, 3, 300, 5
    x = np.float32(np.random.default_rng(14).standard_normal((n, V, Cn)))
    x[:, :, 270] = x[:, :, 7] = np.float32([[4.0, 5.5, 3.25], [6.0, 2.5, 4.75]])
    x[:, :, 131] = x[:, :, 130]
    got = _call(x, [270, 131], k)
    assert got["top_idx"][:, :2].tolist() == [[7, 270]] * 2 and got["rank"].tolist()[0] == 1
    p = _bits(got["prob"])
    assert (p[:, 7] == p[:, 270]).all() and (p[:, 130] == p[:, 131]).all()
    assert (_bits(got["top_val"])[:, 0] == _bits(got["top_val"])[:, 1]).all()
    own = np.argsort(-got["prob"], axis=1, kind="stable")       # the order of the kernel's own float32 p
    assert own[1].tolist().index(131) == got["rank"][1] == own[1].tolist().index(130) + 1


def test_labels_outside_the_classes_form_no_address():
    x, _, k, _, _, _ = _seeded(3, 2, 257)
    good = _call(x, [0, 1, 2], k)
    bad = _call(x, [-1, 257, 2 ** 31 - 1], k)                   # (_call checks the guard words of every output)
    assert bad["rc"] == 0 and bad["rank"].tolist() == [257] * 3 and bad["hits"].tolist() == [3, 0, 0, 3]
    for name in ("top_idx", "top_val", "prob"):
        assert (_bits(bad[name]) == _bits(good[name])).all(), name


def test_the_two_forms_return_the_same_bits(monkeypatch):
    """an image's logits are staged in LDS where they fit 48 KiB and re-read from global memory otherwise
    (Y2_SCORE_NO_STAGE=1: always re-read): the same operations, the same bits; and a shape that does not fit"""
    for shape in ((3, 10, 1000), (2, 16, 256), (1, 3, 5)):
        x, labels, k, _, _, _ = _seeded(*shape)
        monkeypatch.delenv("Y2_SCORE_NO_STAGE", raising=False)
        staged = _call(x, labels, k)
        monkeypatch.setenv("Y2_SCORE_NO_STAGE", "1")
        plain = _call(x, labels, k)
        for name in ("top_idx", "top_val", "prob", "rank", "hits"):
            assert (_bits(staged[name]) == _bits(plain[name])).all(), (shape, name)
    monkeypatch.delenv("Y2_SCORE_NO_STAGE", raising=False)
    n, V, Cn, k = 2, 16, 800, 5                                  # 51,200 bytes of logits per image: not staged
    x = np.float32(3 * np.random.default_rng([0, V, Cn]).standard_normal((n, V, Cn)))
    labels = [5, 799]
    got = _call(x, labels, k)
    rprob = _ref(x, labels, views=V, k=k)[4]
    x64 = x.astype(np.float64)
    bound = (2 * float((x64.max(axis=2, keepdims=True) - x64).max()) + Cn + V + 8) * U
    assert (np.abs(got["prob"] - rprob) / rprob).max() <= bound
    own = np.argsort(-got["prob"], axis=1, kind="stable")
    assert (got["top_idx"] == own[:, :k]).all() and (got["top_val"] == np.take_along_axis(got["prob"], own[:, :k], 1)).all()
    assert (got["rank"] == [own[b].tolist().index(labels[b]) for b in range(n)]).all() and got["hits"][0] == n


def test_every_refusal_is_an_argument_error_without_a_launch():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    n, V, Cn, k = 2, 2, 8, 5
    x = torch.zeros((n * V, Cn), dtype=torch.float32, device="cuda")
    lab = torch.zeros(n, dtype=torch.int32, device="cuda")
    outs = {name: torch.full((64,), 7777, dtype=dt, device="cuda")
            for name, dt in (("prob", torch.float32), ("idx", torch.int32), ("val", torch.float32),
                             ("rank", torch.int32), ("hits", torch.int32))}
    X, LB = _ptr(x), _ptr(lab)
    P, I, VL, R, H = (_ptr(outs[name]) for name in ("prob", "idx", "val", "rank", "hits"))
    calls = [
        (None, LB, n, V, Cn, k, n, P, I, VL, R, H, None),       # null logits / top_idx / top_val
        (X, LB, n, V, Cn, k, n, P, None, VL, R, H, None),
        (X, LB, n, V, Cn, k, n, P, I, None, R, H, None),
        (X, LB, 0, V, Cn, k, 0, P, I, VL, R, H, None),          # n < 1
        (X, LB, -1, V, Cn, k, 0, P, I, VL, R, H, None),
        (X, LB, n, 0, Cn, k, n, P, I, VL, R, H, None),          # views outside 1..16
        (X, LB, n, 17, Cn, k, n, P, I, VL, R, H, None),
        (X, LB, n, V, 0, k, n, P, I, VL, R, H, None),           # classes < 1
        (X, LB, n, V, Cn, 0, n, P, I, VL, R, H, None),          # k outside 1..8
        (X, LB, n, V, Cn, 9, n, P, I, VL, R, H, None),
        (X, LB, n, V, Cn, k, -1, P, I, VL, R, H, None),         # n_valid outside 0..n
        (X, LB, n, V, Cn, k, n + 1, P, I, VL, R, H, None),
        (X, None, n, V, Cn, k, n, P, I, VL, R, None, None),     # rank or hits without labels
        (X, None, n, V, Cn, k, n, P, I, VL, None, H, None),
    ]
    for args in calls:
        assert lib.y2_score_views(*args) == -1, args[2:7]       # Y2_ERR_ARG
        assert b"y2_score_views" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert all((t == 7777).all() for t in outs.values())
    assert lib.y2_score_views(X, None, n, V, Cn, k, 0, None, I, VL, None, None, None) == 0
    torch.cuda.synchronize()
    assert outs["idx"][:n * k].cpu().numpy().reshape(n, k).tolist() == [[0, 1, 2, 3, 4]] * 2
