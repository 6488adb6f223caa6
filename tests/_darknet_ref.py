"""A numpy restatement of what Darknet computes for yolov2-voc.cfg, in float64 and in Darknet's own layout ([C][H][W]),
written from the arrays of a `.weights` file (utils/darknet_weights.split) and sharing no code with the importer:

    convolutional   conv without bias (zero padding k / 2), then with batch_normalize=1
                    (x - rolling_mean) / sqrt(rolling_variance + .000001) * scales + biases, else x + biases;
                    activation leaky (x > 0 ? x : .1 x) or linear
    maxpool         size 2, stride 2
    reorg           utils/darknet_reorg.reorg_darknet_chw, Darknet's four loops
    route           layers=-1,-4: the reorganised map, then the 13x13 path

Test helper only: the tests of the Darknet import compare the device and the importer's arithmetic with it."""
import numpy as np

from tensorflow_yolo2_amd.utils.darknet_reorg import reorg_darknet_chw

POOL_AFTER = (0, 1, 4, 7)        # Darknet-19's max pools inside the stem; the fifth follows layer 12, beside the route


def conv_chw(x, w):
    """x [C][H][W], w [n][c][k][k] -> [n][H][W]: stride 1, zero padding k / 2, no bias"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    n, c, k, _ = w.shape
    assert x.shape[0] == c, (x.shape, w.shape)
    pad = k // 2
    H, W = x.shape[1:]
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad)))
    out = np.zeros((n, H, W), np.float64)
    for dy in range(k):
        for dx in range(k):
            out += np.einsum("nc,chw->nhw", w[:, :, dy, dx], xp[:, dy:dy + H, dx:dx + W])
    return out


def conv_layer(x, d, leaky=True, activate=True):
    """one [convolutional] section on the arrays of its file entry; activate=False stops in front of the activation"""
    col = lambda key: np.asarray(d[key], np.float64)[:, None, None]
    y = conv_chw(x, d["weights"])
    if "scales" in d:
        y = (y - col("rolling_mean")) / np.sqrt(col("rolling_variance") + .000001) * col("scales")
    y = y + col("biases")
    if not activate or not leaky:
        return y
    return np.where(y > 0, y, .1 * y)


def maxpool_chw(x):
    C, H, W = x.shape
    return x.reshape(C, H // 2, 2, W // 2, 2).max(axis=(2, 4))


def yolov2_voc_forward(layers, x):
    """layers: the 23 file entries of yolov2-voc.cfg; x [3][size][size] RGB in [0, 1] -> [B * (5 + C)][S][S]"""
    assert len(layers) == 23
    for l in range(13):
        x = conv_layer(x, layers[l])
        if l in POOL_AFTER:
            x = maxpool_chw(x)
    fine = x                                             # layer 16 of the cfg: 26 x 26 x 512
    x = maxpool_chw(fine)
    for l in range(13, 20):
        x = conv_layer(x, layers[l])
    route = reorg_darknet_chw(conv_layer(fine, layers[20]))
    x = np.concatenate([route, x], axis=0)               # route layers=-1,-4
    x = conv_layer(x, layers[21])
    return conv_layer(x, layers[22], leaky=False)


def random_layers(file_layers, seed):
    """a random weight set with Darknet's semantics for [(k, c, n, batch_norm)]: variances in [0.5, 2], scales near 1,
    filters scaled so that activations stay of order one"""
    rng = np.random.default_rng(seed)
    out = []
    for (k, c, n, bn) in file_layers:
        d = {"biases": rng.normal(0, 0.2, n).astype(np.float32)}
        if bn:
            d["scales"] = rng.uniform(0.8, 1.2, n).astype(np.float32)
            d["rolling_mean"] = rng.normal(0, 0.2, n).astype(np.float32)
            d["rolling_variance"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
        d["weights"] = rng.normal(0, np.sqrt(2.0 / (c * k * k)), (n, c, k, k)).astype(np.float32)
        out.append(d)
    return out
