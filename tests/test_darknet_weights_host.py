"""Host tests (no GPU) of the Darknet import: the `.weights` format (utils/darknet_weights.py), Darknet's reorg
(utils/darknet_reorg.py), the per-layer fold arithmetic in float64 against tests/_darknet_ref.py, and the first-layer
fold of read_darknet_backbone with its border ring."""
import struct

import numpy as np
import pytest

import _darknet_ref as D
from tensorflow_yolo2_amd.utils import darknet_reorg as RG
from tensorflow_yolo2_amd.utils import darknet_weights as DW

LAYERS = [(3, 2, 4, True), (1, 4, 3, False)]         # one batch-norm layer (k 3, 2 -> 4) and one plain (k 1, 4 -> 3)
N_FLOATS = (4 * 4 + 4 * 2 * 9) + (3 + 3 * 4)


def _packed(path, major, minor, seen_fmt, seen, values):
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", major, minor, 0))
        f.write(struct.pack(seen_fmt, seen))
        f.write(struct.pack("<%df" % len(values), *values))


def _values():
    return [float(np.float32(0.25 * i - 7.0)) for i in range(N_FLOATS)]


# ---------------------------------------------------------------- 1. format
@pytest.mark.parametrize("major,minor,fmt,seen", [(0, 1, "<i", 12800), (0, 2, "<Q", 2 ** 33 + 5)])
def test_reader_parses_a_file_packed_by_hand(tmp_path, major, minor, fmt, seen):
    path = str(tmp_path / "hand.weights")
    vals = _values()
    _packed(path, major, minor, fmt, seen, vals)
    mj, mn, rev, got_seen, arr = DW.read(path)
    assert (mj, mn, rev, got_seen) == (major, minor, 0, seen)
    assert arr.dtype == np.float32 and arr.size == N_FLOATS
    layers, used = DW.split(arr, LAYERS)
    assert used == N_FLOATS and len(layers) == 2
    v = np.asarray(vals, np.float32)
    np.testing.assert_array_equal(layers[0]["biases"], v[0:4])
    np.testing.assert_array_equal(layers[0]["scales"], v[4:8])
    np.testing.assert_array_equal(layers[0]["rolling_mean"], v[8:12])
    np.testing.assert_array_equal(layers[0]["rolling_variance"], v[12:16])
    assert layers[0]["weights"].shape == (4, 2, 3, 3)
    np.testing.assert_array_equal(layers[0]["weights"], v[16:88].reshape(4, 2, 3, 3))
    assert sorted(layers[1]) == ["biases", "weights"]
    np.testing.assert_array_equal(layers[1]["biases"], v[88:91])
    np.testing.assert_array_equal(layers[1]["weights"], v[91:103].reshape(3, 4, 1, 1))


@pytest.mark.parametrize("major,minor,seen", [(0, 1, 7), (0, 2, 2 ** 40 + 1)])
def test_write_then_read_is_bit_identical(tmp_path, major, minor, seen):
    layers = D.random_layers(LAYERS, 3)
    layers[0]["weights"][0, 0, 0, 0] = np.float32(-0.0)
    layers[1]["biases"][1] = np.float32(1e-42)                 # a denormal keeps its bits too
    path = str(tmp_path / "w.weights")
    DW.write(path, layers, seen, major, minor, 4)
    mj, mn, rev, got_seen, arr = DW.read(path)
    assert (mj, mn, rev, got_seen) == (major, minor, 4, seen)
    back, used = DW.split(arr, LAYERS)
    assert used == N_FLOATS
    for a, b in zip(layers, back):
        assert sorted(a) == sorted(b)
        for k in a:
            np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
    path2 = str(tmp_path / "w2.weights")
    DW.write(path2, back, got_seen, mj, mn, rev)
    assert open(path, "rb").read() == open(path2, "rb").read()


def test_prefix_file_and_refusals(tmp_path):
    arr = np.asarray(_values(), np.float32)
    first = DW.layer_floats(LAYERS[0])
    assert first == 88
    layers, used = DW.split(arr[:first], LAYERS)               # ends at a layer boundary: a `.conv.N` file
    assert len(layers) == 1 and used == first
    with pytest.raises(ValueError) as e:
        DW.split(arr[:first + 5], LAYERS)                      # cut inside layer 1: 15 needed, 5 left
    assert "layer 1" in str(e.value) and "15" in str(e.value) and "5" in str(e.value)
    with pytest.raises(ValueError) as e:
        DW.split(arr[:40], LAYERS)                             # cut inside layer 0: 88 needed, 40 left
    assert "layer 0" in str(e.value) and "88" in str(e.value) and "40" in str(e.value)
    with pytest.raises(ValueError) as e:
        DW.split(np.concatenate([arr, np.zeros(1, np.float32)]), LAYERS)
    assert "1 floats are left" in str(e.value) and str(N_FLOATS) in str(e.value)


def test_yolov2_voc_layer_list():
    layers = DW.yolov2_voc_layers(20, 5)
    assert len(layers) == 23 and [l[3] for l in layers] == [True] * 22 + [False]
    assert layers[3] == (1, 128, 64, True) and layers[20] == (1, 512, 64, True)
    assert layers[21] == (3, 1280, 1024, True) and layers[22] == (1, 1024, 125, False)
    assert sum(DW.layer_floats(l) for l in layers) == 50676061          # yolov2-voc.weights: 202,704,260 bytes - 16


# ---------------------------------------------------------------- 2. reorg
@pytest.mark.parametrize("shape", [(2, 4, 6, 8), (1, 2, 2, 4), (1, 26, 26, 64)])
def test_reorg_loop_form_equals_the_index_table(shape):
    n, H, W, C = shape
    fine = np.arange(n * H * W * C, dtype=np.float32).reshape(shape)          # distinct values
    got = RG.reorg_darknet(fine)
    assert got.shape == (n, H // 2, W // 2, 4 * C)
    for b in range(n):
        ref = RG.reorg_darknet_chw(fine[b].transpose(2, 0, 1))                # [4C][H/2][W/2]
        np.testing.assert_array_equal(got[b], ref.transpose(1, 2, 0))
        # a bijection of each image
        np.testing.assert_array_equal(np.sort(got[b].reshape(-1)), np.sort(fine[b].reshape(-1)))
    js, is_, cs = RG.reorg_darknet_table(H, W, C)
    flat = (js * W + is_) * C + cs
    assert np.unique(flat).size == H * W * C


def test_reorg_is_not_the_space_to_depth():
    from oracle import ext_ref as X
    fine = np.arange(26 * 26 * 64, dtype=np.float32).reshape(1, 26, 26, 64)
    a, b = RG.reorg_darknet(fine), X.reorg(fine)
    assert a.shape == b.shape and not np.array_equal(a, b)
    # and no permutation of channels turns one into the other: a pixel of Darknet's output mixes input pixels that the
    # space-to-depth keeps apart
    js, is_, _cs = RG.reorg_darknet_table(26, 26, 64)
    blocks = set(zip((js[0, 0] // 2).tolist(), (is_[0, 0] // 2).tolist()))
    assert len(blocks) > 1


# ---------------------------------------------------------------- 3. fold arithmetic, float64
def _repo_layer(x, p, eps, slope):
    """this repository's layer on a dict: act(gamma * (conv(x, W) + b - mean) / sqrt(var + eps) + beta), NHWC float64"""
    from oracle import nn_ref as R
    f = lambda k: np.asarray(p[k], np.float64)
    h = R.conv2d_same(np.asarray(x, np.float64), f("W")) + f("b")
    y = f("gamma") * (h - f("moving_mean")) / np.sqrt(f("moving_var") + eps) + f("beta")
    return np.where(y > 0, y, slope * y)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("k_file,k_model,bn", [(3, 3, True), (1, 1, True), (1, 3, True), (1, 1, False), (3, 3, False)])
def test_import_fold_matches_darknet_layer(k_file, k_model, bn):
    rng = np.random.default_rng(10 * k_file + k_model + bn)
    c, n = 6, 5
    d = D.random_layers([(k_file, c, n, bn)], 5 + k_file + k_model)[0]
    x = rng.standard_normal((c, 7, 9))
    ref = D.conv_layer(x, d, leaky=bn)                                   # the plain layer is the cfg's linear last one
    p = DW.to_layer_params(d, k_model, 1e-6, dtype=np.float64)
    assert p["W"].shape == (k_model, k_model, c, n)
    got = _repo_layer(x.transpose(1, 2, 0)[None], p, 1e-6, 0.1 if bn else 1.0)[0].transpose(2, 0, 1)
    assert _rel(got, ref) <= 1e-12
    if not bn:      # the identity batch norm of the last layer, on its own
        h = rng.standard_normal((4, n))
        y = p["gamma"] * (h - p["moving_mean"]) / np.sqrt(p["moving_var"] + 1e-6) + p["beta"]
        assert _rel(y, h) <= 1e-12
        # in float32 it is the identity to one ulp
        p32 = DW.to_layer_params(d, k_model, 1e-6)
        assert p32["gamma"].dtype == np.float32 and abs(float(p32["gamma"][0]) / np.sqrt(1 + 1e-6) - 1) < 2.0 ** -24


@pytest.mark.parametrize("k_file,k_model,bn", [(3, 3, True), (1, 3, True), (1, 1, False)])
def test_export_fold_matches_repository_layer(k_file, k_model, bn):
    rng = np.random.default_rng(77 + k_file + k_model + bn)
    c, n = 6, 5
    W = rng.standard_normal((k_file, k_file, c, n)) * 0.3
    if k_model != k_file:
        full = np.zeros((3, 3, c, n))
        full[1, 1] = W[0, 0]
        W = full
    p = {"W": W, "b": rng.normal(0, 0.5, n), "gamma": rng.uniform(0.5, 1.5, n), "beta": rng.normal(0, 0.3, n),
         "moving_mean": rng.normal(0, 0.5, n), "moving_var": rng.uniform(0.5, 2.0, n)}
    x = rng.standard_normal((c, 8, 6))
    ref = _repo_layer(x.transpose(1, 2, 0)[None], p, 1e-6, 0.1 if bn else 1.0)[0].transpose(2, 0, 1)
    d = DW.from_layer_params(p, k_file, bn, 1e-6, dtype=np.float64)
    assert d["weights"].shape == (n, c, k_file, k_file) and ("scales" in d) == bn
    assert _rel(D.conv_layer(x, d, leaky=bn), ref) <= 1e-12


def test_export_of_an_imported_layer_returns_its_bits():
    for (k_file, k_model, bn) in [(3, 3, True), (1, 3, True), (1, 1, False)]:
        d = D.random_layers([(k_file, 6, 5, bn)], 31 + k_file)[0]
        back = DW.from_layer_params(DW.to_layer_params(d, k_model, 1e-6), k_file, bn, 1e-6)
        assert sorted(back) == sorted(d)
        for k in d:
            assert back[k].dtype == np.float32
            np.testing.assert_array_equal(back[k].view(np.uint32), d[k].view(np.uint32))
    p = DW.to_layer_params(D.random_layers([(1, 6, 5, True)], 2)[0], 3, 1e-6)
    p["W"][0, 2, 1, 1] = 0.5
    with pytest.raises(ValueError):                      # a trained off-centre tap cannot go back into a 1x1 filter
        DW.from_layer_params(p, 1, True, 1e-6)


# ---------------------------------------------------------------- 4. the first layer of read_darknet_backbone
@pytest.mark.parametrize("dtype,per_element", [(np.float64, True), (np.float32, False)])
def test_first_layer_fold_is_exact_inside_and_not_on_the_ring(dtype, per_element):
    rng = np.random.default_rng(12)
    img = rng.integers(0, 256, (12, 12, 3), dtype=np.uint8)            # BGR pixels
    d = D.random_layers([(3, 3, 8, True)], 9)[0]
    x_darknet = (img[:, :, ::-1].astype(np.float64) / 255.0).transpose(2, 0, 1)          # RGB in [0, 1], zero = black
    ref = D.conv_layer(x_darknet, d)
    p = DW.fold_first_layer(DW.to_layer_params(d, 3, 1e-6, dtype=dtype), dtype=dtype)
    np.testing.assert_array_equal(p["W"], (DW.to_layer_params(d, 3, 1e-6, dtype=dtype)["W"][:, :, ::-1, :] * 0.5))
    x_here = img.astype(np.float64) / 255.0 * 2.0 - 1.0                                  # BGR in [-1, 1), zero = mid-grey
    got = _repo_layer(x_here[None], p, 1e-6, 0.1)[0].transpose(2, 0, 1)
    inner = (slice(None), slice(1, -1), slice(1, -1))
    if per_element:
        np.testing.assert_allclose(got[inner], ref[inner], rtol=1e-6, atol=0)            # every interior pixel
    else:       # the float32 arrays the importer hands on: the rounding of the folded mean, against the layer's scale
        assert np.abs(got[inner] - ref[inner]).max() <= 1e-6 * np.abs(ref[inner]).max()
    ring = np.ones(ref.shape, bool)
    ring[inner] = False
    assert np.abs(got[ring] - ref[ring]).max() > 1e-3 * np.abs(ref).max()                # the exclusion is not vacuous
