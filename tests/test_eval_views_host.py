"""Host tests (no GPU) of the evaluation views (img_dataset/eval_views.py) and of the scoring specification
(utils/score_views.py): geometries whose weights are 0, so that a view is an exact copy of source bytes; the long side's
rule; every argument error; and hand-made scoring cases."""
import numpy as np
import pytest


def _EV():
    from tensorflow_yolo2_amd.img_dataset import eval_views
    return eval_views


def _ref():
    from tensorflow_yolo2_amd.utils.score_views import score_views_ref
    return score_views_ref


def _img(h, w, seed=3):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- views
def test_centre_of_a_tall_and_of_a_wide_image_is_the_exact_crop():
    EV = _EV()
    tall = _img(40, 32)
    rows = EV.view_rows([(40, 32)], 32, "centre")
    assert rows.shape == (1, 1, 9) and rows.dtype == np.float64
    assert (EV.view_images(tall, rows[0], 32) == tall[4:36][None]).all()
    wide = _img(32, 48)
    rows = EV.view_rows([(32, 48)], 32, "centre")
    got = EV.view_images(wide, rows[0], 32)
    assert got.shape == (1, 32, 32, 3) and got.dtype == np.uint8 and (got[0] == wide[:, 8:40]).all()
    assert (rows[..., 6:] == (0.0, 1.0, 1.0)).all()


def test_ten_views_of_a_square_image_are_its_corner_blocks_the_centre_and_their_mirrors():
    EV = _EV()
    img = _img(64, 64)
    rows = EV.view_rows([(64, 64)], 32, "ten", margin=32)
    assert rows.shape == (1, 10, 9) and (rows[..., 6:] == (0.0, 1.0, 1.0)).all()
    got = EV.view_images(img, rows[0], 32)
    blocks = lambda a: [a[:32, :32], a[:32, 32:], a[32:, :32], a[32:, 32:], a[16:48, 16:48]]
    for v, want in enumerate(blocks(img) + blocks(img[:, ::-1])):
        assert (got[v] == want).all(), v


def test_stretch_rows_are_the_identity_rows():
    EV = _EV()
    from tensorflow_yolo2_amd.img_dataset.augment_cls import identity_row
    shapes = [(40, 52), (64, 48), (33, 33), (1, 7)]
    rows = EV.view_rows(shapes, 64, "stretch")
    assert rows.shape == (4, 1, 9)
    for b, (h, w) in enumerate(shapes):
        assert (rows[b, 0] == identity_row(h, w, 64)).all()
    assert EV.VIEWS == {"stretch": 1, "centre": 1, "ten": 10}


@pytest.mark.parametrize("hw", [(375, 500), (500, 333)])
def test_the_long_side_is_the_truncated_product(hw):
    """scaled long side = int(long * (L / short)); recovered from the row: m00 = W / scaled_w, m11 = H / scaled_h, and the
    centre offset from m02, m12"""
    EV = _EV()
    from tensorflow_yolo2_amd.img_dataset.augment_cls import compose
    H, W = hw
    for views, L in (("centre", 224.0), ("ten", 256.0)):
        short, long_ = min(H, W), max(H, W)
        scaled_long = float(int(long_ * (L / short)))
        sw, sh = (scaled_long, L) if W > H else (L, scaled_long)
        assert (sw, sh) == {(375, 500, 224.0): (298.0, 224.0), (500, 333, 224.0): (224.0, 336.0),
                            (375, 500, 256.0): (341.0, 256.0), (500, 333, 256.0): (256.0, 384.0)}[(H, W, L)]
        rows = EV.view_rows([hw], 224, views, margin=32)
        centre = rows[0, -1 if views == "centre" else 4]
        want = compose(H, W, sw, sh, (sw - 224) // 2, (sh - 224) // 2, 0.0, False)
        assert (centre[:6] == want).all()
        if views == "ten":
            offs = [(0, 0), (sw - 224, 0), (0, sh - 224), (sw - 224, sh - 224), ((sw - 224) // 2, (sh - 224) // 2)]
            for v in range(10):
                ox, oy = offs[v % 5]
                assert (rows[0, v, :6] == compose(H, W, sw, sh, ox, oy, 0.0, v >= 5)).all(), v


def test_a_square_image_whose_rounded_product_falls_short_keeps_its_crop_inside():
    """49 * (32 / 49) < 32 in float64: the long side stays L and the centre view is the plain stretch"""
    EV = _EV()
    from tensorflow_yolo2_amd.img_dataset.augment_cls import compose
    assert np.floor(49.0 * (32.0 / 49.0)) == 31.0
    rows = EV.view_rows([(49, 49)], 32, "centre")
    assert (rows[0, 0, :6] == compose(49, 49, 32.0, 32.0, 0, 0, 0.0, False)).all()


def test_every_argument_error_of_the_views():
    EV = _EV()
    with pytest.raises(ValueError, match="views"):
        EV.view_rows([(40, 32)], 32, "five")
    for size in (0, -32, 48, 31):
        with pytest.raises(ValueError, match="multiple of 32"):
            EV.view_rows([(40, 32)], size, "centre")
    with pytest.raises(ValueError, match="margin"):
        EV.view_rows([(40, 32)], 32, "ten", margin=-1)
    for shape in ((0, 32), (40, 0), (-1, 5)):
        with pytest.raises(ValueError, match="side below 1"):
            EV.view_rows([(40, 32), shape], 32, "centre")
    assert EV.view_rows([(40, 32)], 32, "ten", margin=0).shape == (1, 10, 9)


# ---- scoring specification
def test_ref_ties_go_to_the_lower_index():
    ref = _ref()
    x = np.array([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0]])
    idx, val, rank, hits, prob = ref(x, labels=[4], views=1, k=3)
    assert idx.tolist() == [[1, 2, 4]] and rank.tolist() == [2] and hits.tolist() == [1, 0, 1, 0]
    assert val[0, 0] == val[0, 1] == val[0, 2] == prob[0, 1]
    np.testing.assert_allclose(prob.sum(axis=1), 1.0, rtol=1e-15)
    # two views: the order is that of the mean probability; classes 0 and 2 tie exactly, 0 comes first
    x2 = np.array([[0.0, 1.0, 0.0], [0.0, -3.0, 0.0]])
    idx, val, rank, hits, prob = ref(x2, labels=[2], views=2, k=2)
    e = np.exp(np.array([0.0, 1.0, 0.0]) - 1.0)
    f = np.exp(np.array([0.0, -3.0, 0.0]))
    want = 0.5 * (e / e.sum() + f / f.sum())
    np.testing.assert_allclose(prob[0], want, rtol=1e-15)
    assert prob[0, 0] == prob[0, 2] > prob[0, 1]
    assert idx.tolist() == [[0, 2]] and rank.tolist() == [1] and hits.tolist() == [1, 0, 1, 0]


def test_ref_pads_when_there_are_fewer_classes_than_k():
    ref = _ref()
    idx, val, rank, hits, prob = ref(np.array([[0.5, 2.0, 1.0]]), labels=[0], views=1, k=5)
    assert idx.tolist() == [[1, 2, 0, -1, -1]] and val[0, 3:].tolist() == [0.0, 0.0]
    assert rank.tolist() == [2] and hits.tolist() == [1, 0, 1, 0]
    idx, val, rank, hits, _ = ref(np.array([[7.0]]), labels=[0], views=1, k=1)
    assert idx.tolist() == [[0]] and val.tolist() == [[1.0]] and rank.tolist() == [0] and hits.tolist() == [1, 1, 1, 0]


def test_ref_label_outside_the_classes_is_a_counted_miss():
    ref = _ref()
    x = np.array([[0.5, 2.0, 1.0]] * 4)
    idx, val, rank, hits, prob = ref(x, labels=[-1, 3, 2 ** 31 - 1, 1], views=1, k=5)
    assert rank.tolist() == [3, 3, 3, 0]
    assert hits.tolist() == [4, 1, 1, 3]                        # (3 < k = 5, and still no top-k hit)
    good = ref(x, labels=[1, 1, 1, 1], views=1, k=5)
    assert (idx == good[0]).all() and (val == good[1]).all() and (prob == good[4]).all()


def test_ref_n_valid_masks_the_counters_alone_and_hits_accumulate():
    ref = _ref()
    x = np.random.default_rng(1).standard_normal((6, 7))
    labels = [0, 6, 2]
    full = ref(x, labels=labels, views=2, k=2)
    part = ref(x, labels=labels, views=2, k=2, n_valid=1, hits=[10, 5, 7, 1])
    for a, b in zip(full[:3] + full[4:], part[:3] + part[4:]):
        assert (a == b).all()
    first = ref(x[:2], labels=labels[:1], views=2, k=2)[3]
    assert part[3].tolist() == (np.array([10, 5, 7, 1]) + first).tolist() and first[0] == 1 and full[3][0] == 3
    assert ref(x, labels=labels, views=2, k=2, n_valid=0)[3].tolist() == [0, 0, 0, 0]
    assert ref(x, views=2)[2:4] == (None, None)
    for bad in (dict(views=0), dict(views=17), dict(k=0), dict(k=9), dict(views=4), dict(n_valid=4, views=2)):
        with pytest.raises(ValueError):
            ref(x, **bad)
