"""Darknet's `.weights` files (numpy only): the reader, the splitter into per-layer arrays and the writer.

Layout, little endian.  Header: int32 `major`, `minor`, `revision`, then `seen` (the images the run had trained on) --
uint64 if `major * 10 + minor >= 2` and `major < 1000` and `minor < 1000`, else int32 -- then float32 values to the end
of the file.  Per convolution, in the order of the cfg:

    with batch norm     biases[n] (the BN shift)  scales[n]  rolling_mean[n]  rolling_variance[n]  weights[n][c][k][k]
    without             biases[n]  weights[n][c][k][k]

A layer is `(k, c, n, batch_norm)`: filter size, input channels, filters, whether the cfg line has `batch_normalize=1`.
`yolov2_voc_layers` is the list of yolov2-voc.cfg; its first 18 entries are the list of `darknet19_448.conv.23`, a file
that ends at a layer boundary -- `split` takes such a prefix and refuses a file that ends anywhere else."""
import struct

import numpy as np

BN_KEYS = ("biases", "scales", "rolling_mean", "rolling_variance", "weights")
PLAIN_KEYS = ("biases", "weights")

# (filter size, in, out) of the 18 Darknet-19 core convolutions (darknet19_448.cfg up to its 23rd layer)
DARKNET19_CORE = (
    (3, 3, 32), (3, 32, 64), (3, 64, 128), (1, 128, 64), (3, 64, 128), (3, 128, 256), (1, 256, 128), (3, 128, 256),
    (3, 256, 512), (1, 512, 256), (3, 256, 512), (1, 512, 256), (3, 256, 512),
    (3, 512, 1024), (1, 1024, 512), (3, 512, 1024), (1, 1024, 512), (3, 512, 1024),
)


def yolov2_voc_layers(num_class=20, num_anchors=5):
    """the 23 convolutions of yolov2-voc.cfg as (k, c, n, batch_norm), in file order"""
    layers = [(k, c, n, True) for (k, c, n) in DARKNET19_CORE]
    layers += [(3, 1024, 1024, True), (3, 1024, 1024, True), (1, 512, 64, True), (3, 4 * 64 + 1024, 1024, True),
               (1, 1024, num_anchors * (5 + num_class), False)]
    return layers


def yolov2_tiny_voc_layers(num_class=20, num_anchors=5):
    """the 9 convolutions of tiny-yolo-voc.cfg (yolov2-tiny-voc.cfg) as (k, c, n, batch_norm), in file order: 15,867,885
    floats at 20 classes and 5 anchors -- with the 16-byte header the 63,471,556 bytes of tiny-yolo-voc.weights"""
    widths = (3, 16, 32, 64, 128, 256, 512, 1024, 1024)
    layers = [(3, c, n, True) for c, n in zip(widths[:-1], widths[1:])]
    return layers + [(1, 1024, num_anchors * (5 + num_class), False)]


def seen_is_64bit(major, minor):
    return major * 10 + minor >= 2 and major < 1000 and minor < 1000


def layer_floats(layer):
    k, c, n, bn = layer
    return n * c * k * k + (4 * n if bn else n)


def read(path):
    """-> (major, minor, revision, seen, float32 array of every value behind the header)"""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 16:
        raise ValueError("%s: %d bytes is shorter than a Darknet header" % (path, len(data)))
    major, minor, revision = struct.unpack_from("<iii", data, 0)
    if seen_is_64bit(major, minor):
        if len(data) < 20:
            raise ValueError("%s: %d bytes is shorter than a Darknet header with a 64-bit seen" % (path, len(data)))
        seen, off = struct.unpack_from("<Q", data, 12)[0], 20
    else:
        seen, off = struct.unpack_from("<i", data, 12)[0], 16
    if (len(data) - off) % 4:
        raise ValueError("%s: %d bytes behind the header is no whole number of float32" % (path, len(data) - off))
    return major, minor, revision, int(seen), np.frombuffer(data, "<f4", offset=off).astype(np.float32)


def split(array, layers):
    """array: the float32 values of a file; layers: [(k, c, n, batch_norm)] -> ([dict of Darknet's arrays per layer],
    floats used).  Fewer dicts than layers come back when the values end exactly at a layer boundary (a `.conv.23`
    file); ValueError when they end inside a layer or go on behind the last one."""
    array = np.asarray(array, np.float32).reshape(-1)
    out, pos = [], 0
    for l, layer in enumerate(layers):
        if pos == array.size:
            break
        k, c, n, bn = layer
        need = layer_floats(layer)
        if array.size - pos < need:
            raise ValueError("Darknet weights end inside layer %d (k %d, %d -> %d%s): it needs %d floats, %d are left" %
                             (l, k, c, n, ", batch norm" if bn else "", need, array.size - pos))
        d = {}
        for key in (BN_KEYS if bn else PLAIN_KEYS)[:-1]:
            d[key] = array[pos:pos + n].copy()
            pos += n
        d["weights"] = array[pos:pos + n * c * k * k].reshape(n, c, k, k).copy()
        pos += n * c * k * k
        out.append(d)
    if pos != array.size:
        raise ValueError("Darknet weights: %d floats are left behind layer %d, the last of the list (%d used of %d)" %
                         (array.size - pos, len(layers) - 1, pos, array.size))
    return out, pos


# ---------------------------------------------------------------------------
# Between Darknet's arrays and this repository's layer dicts (W [k][k][c][n], b, gamma, beta, moving_mean, moving_var;
# the layer computes leaky(gamma * (conv(x, W) + b - moving_mean) / sqrt(moving_var + eps) + beta)).  numpy only: the
# device side is yolo2_nets/net_utils.load_darknet_weights / save_darknet_weights / read_darknet_backbone.
# ---------------------------------------------------------------------------
def _filters_in(weights, k_model, dtype):
    """Darknet's [n][c][k][k] -> [k][k][c][n]; a 1x1 filter for a 3x3 layer sits on the centre tap, the other eight are
    zero -- the same function under zero padding (this repository's Darknet-19 runs its fourth layer as 3x3, the
    reference's graph, where Darknet's is 1x1)"""
    w = np.asarray(weights, dtype).transpose(2, 3, 1, 0)
    k = w.shape[0]
    if k == k_model:
        return np.ascontiguousarray(w)
    if k != 1 or k_model != 3:
        raise ValueError("a %dx%d Darknet filter does not fit a %dx%d layer" % (k, k, k_model, k_model))
    out = np.zeros((3, 3) + w.shape[2:], dtype)
    out[1, 1] = w[0, 0]
    return out


def _filters_out(W, k_file, dtype):
    W = np.asarray(W, dtype)
    if W.shape[0] != k_file:
        if W.shape[0] != 3 or k_file != 1:
            raise ValueError("a %dx%d layer does not fit a %dx%d Darknet filter" % (W.shape[0], W.shape[0], k_file, k_file))
        off_centre = W.copy()
        off_centre[1, 1] = 0
        if np.any(off_centre != 0):
            raise ValueError("a 3x3 layer written as Darknet's 1x1 needs its eight off-centre taps to be zero")
        W = W[1:2, 1:2]
    return np.ascontiguousarray(W.transpose(3, 2, 0, 1))


def to_layer_params(d, k_model, eps, dtype=np.float32):
    """one dict of `split` -> this repository's layer dict.  Batch norm: the arrays are copied, b = 0.  Without (the last
    layer of yolov2-voc.cfg): b = biases, and the layer's inference batch norm is made the identity -- gamma =
    dtype(sqrt(1 + eps)), beta = 0, mean 0, variance 1: exact in float64, one ulp in float32"""
    W = _filters_in(d["weights"], k_model, dtype)
    n = W.shape[3]
    a = lambda key: np.asarray(d[key], dtype).copy()
    if "scales" in d:
        return {"W": W, "b": np.zeros(n, dtype), "gamma": a("scales"), "beta": a("biases"),
                "moving_mean": a("rolling_mean"), "moving_var": a("rolling_variance")}
    return {"W": W, "b": a("biases"), "gamma": np.full(n, np.sqrt(1.0 + np.float64(eps)), dtype),
            "beta": np.zeros(n, dtype), "moving_mean": np.zeros(n, dtype), "moving_var": np.ones(n, dtype)}


def from_layer_params(p, k_file, batch_norm, eps, dtype=np.float32):
    """the inverse: a layer dict -> Darknet's arrays.  Batch norm: the conv bias folds into the mean, rolling_mean =
    moving_mean - b.  Without: the inference affine s = gamma / sqrt(moving_var + eps) (formed in float64, rounded to
    `dtype`: exactly 1 for what to_layer_params wrote) is folded in, weights = W s per filter, biases = s (b - mean) +
    beta, so a layer that to_layer_params filled comes back with the bits it was read with"""
    g = lambda key: np.asarray(p[key], dtype)
    if batch_norm:
        return {"biases": g("beta").copy(), "scales": g("gamma").copy(), "rolling_mean": g("moving_mean") - g("b"),
                "rolling_variance": g("moving_var").copy(), "weights": _filters_out(p["W"], k_file, dtype)}
    f64 = lambda key: np.asarray(p[key], np.float64)
    s = (f64("gamma") / np.sqrt(f64("moving_var") + np.float64(eps))).astype(dtype).astype(np.float64)
    t = s * (f64("b") - f64("moving_mean"))
    biases = np.where(f64("beta") == 0, t, t + f64("beta")).astype(dtype)        # (a zero beta keeps the sign of -0.0)
    return {"biases": biases, "weights": _filters_out(f64("W") * s, k_file, np.float64).astype(dtype)}


PAD_VALUES = {"b": 0, "gamma": 1, "beta": 0, "moving_mean": 0, "moving_var": 1}


def pad_layer_params(p, c_model, n_model):
    """a layer dict of the file's widths [k][k][c][n] -> the same function at the model's widths c_model >= c, n_model >=
    n (tiny-yolo-voc.cfg's 3 -> 16 and 16 -> 32 in stacks whose widths are multiples of 32): the added filters and input
    channels are zero, the added filters' b = 0, gamma = 1, beta = 0, moving mean 0, moving variance 1.  Under zero
    padding and either batch-norm mode a zero filter's activation is exactly 0 (batch mean 0, variance 0: 0 / sqrt(eps) =
    0), and a zero input channel adds exactly 0 to every sum"""
    W = np.asarray(p["W"])
    k, _k, c, n = W.shape
    if c > c_model or n > n_model:
        raise ValueError("a %d -> %d layer does not fit a %d -> %d one" % (c, n, c_model, n_model))
    if (c, n) == (c_model, n_model):
        return p
    out = {"W": np.zeros((k, k, c_model, n_model), W.dtype)}
    out["W"][:, :, :c, :n] = W
    for key, fill in PAD_VALUES.items():
        a = np.asarray(p[key])
        out[key] = np.concatenate([a, np.full(n_model - n, fill, a.dtype)])
    return out


def strip_layer_params(p, c_file, n_file, check=True):
    """the inverse: the leading c_file input channels and n_file filters of a layer dict.  check: refuse a layer that is
    not the padded form of one -- a non-zero filter value, b, beta or moving mean among the entries that go (gamma and
    the moving variance scale an exact zero: training moves the padded variances, and they may)"""
    W = np.asarray(p["W"])
    _k, _k2, c, n = W.shape
    if c_file > c or n_file > n:
        raise ValueError("a %d -> %d layer holds no %d -> %d one" % (c, n, c_file, n_file))
    if (c, n) == (c_file, n_file):
        return p
    if check:
        gone = W.copy()
        gone[:, :, :c_file, :n_file] = 0
        bad = ["W"] if np.any(gone != 0) else []
        bad += [key for key in ("b", "beta", "moving_mean") if np.any(np.asarray(p[key])[n_file:] != 0)]
        if bad:
            raise ValueError("a %d -> %d layer written as Darknet's %d -> %d needs its padded entries to be zero: %s has "
                             "non-zero ones" % (c, n, c_file, n_file, ", ".join(bad)))
    out = {"W": np.ascontiguousarray(W[:, :, :c_file, :n_file])}
    for key in PAD_VALUES:
        out[key] = np.asarray(p[key])[:n_file].copy()
    return out


def fold_first_layer(p, dtype=np.float32):
    """a first-layer dict made for Darknet's input (RGB in [0, 1]) -> the same layer on this repository's input (BGR in
    [-1, 1): x_darknet[c] = (x[2 - c] + 1) / 2).  The filter channels are reversed and halved (exact) and the constant
    sum(W) / 2 over the taps moves into moving_mean.  Exact wherever all k * k taps lie inside the image; NOT on the
    one-pixel border ring, where Darknet pads with black (-1 here) and this stack with 0, Darknet's mid-grey."""
    W = np.asarray(p["W"], np.float64)
    out = dict(p)
    out["W"] = (W[:, :, ::-1, :] * 0.5).astype(dtype)
    out["moving_mean"] = (np.asarray(p["moving_mean"], np.float64) - 0.5 * W.sum(axis=(0, 1, 2))).astype(dtype)
    return out


def write(path, layers, seen, major=0, minor=1, revision=0):
    """layers: the dicts `split` returns (a layer with `scales` has batch norm) -> the file; `read` of it returns the
    same bits"""
    head = struct.pack("<iii", major, minor, revision)
    head += struct.pack("<Q" if seen_is_64bit(major, minor) else "<i", int(seen))
    parts = []
    for l, d in enumerate(layers):
        keys = BN_KEYS if "scales" in d else PLAIN_KEYS
        w = np.asarray(d["weights"], np.float32)
        if w.ndim != 4 or w.shape[2] != w.shape[3]:
            raise ValueError("layer %d: weights of shape %s are not [n][c][k][k]" % (l, w.shape))
        for key in keys[:-1]:
            a = np.asarray(d[key], np.float32).reshape(-1)
            if a.size != w.shape[0]:
                raise ValueError("layer %d: %s holds %d values for %d filters" % (l, key, a.size, w.shape[0]))
            parts.append(a)
        parts.append(w.reshape(-1))
    body = np.concatenate(parts).astype("<f4") if parts else np.zeros(0, "<f4")
    with open(path, "wb") as f:
        f.write(head)
        f.write(body.tobytes())
    return len(head) + body.nbytes
