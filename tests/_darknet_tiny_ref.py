"""What Darknet computes for tiny-yolo-voc.cfg, restated for the tests of the "tiny" topology from the arrays of a
`.weights` file (utils/darknet_weights.split), sharing no code with the importer:

    tiny_forward    inference in numpy float64 and Darknet's [C][H][W]: nine [convolutional] sections
                    (tests/_darknet_ref.conv_layer), maxpool 2 / 2 behind the first five, maxpool size 2 stride 1 behind
                    the sixth, the last section linear and without batch norm
    Pass            the TRAINING pass in torch float64 autograd, NHWC like the device: batch statistics (mean and biased
                    variance over N, H, W, epsilon .000001) in the eight conv-BN-leaky layers, conv + biases in the last

The stride-1 pool is written here on its own -- the map padded at the bottom and right with -inf, the maximum of the four
shifts -- and not through utils/darknet_maxpool.py.  The file's 16-wide layers stay 16 wide here: the device's padded
layers are compared on their real entries.

Test helper only."""
import numpy as np
import torch
import torch.nn.functional as F

from _darknet_ref import conv_layer, maxpool_chw, random_layers          # noqa: F401  (random_layers: for the tests)

EPS = 1e-6
N_LAYERS = 9


def maxpool_s1_chw(x):
    """x [C][H][W] -> [C][H][W]: Darknet's size 2, stride 1, padding 1 pool: windows anchored top-left, clipped"""
    C, H, W = x.shape
    p = np.full((C, H + 1, W + 1), -np.inf, np.float64)
    p[:, :H, :W] = x
    return np.maximum(np.maximum(p[:, :H, :W], p[:, :H, 1:]), np.maximum(p[:, 1:, :W], p[:, 1:, 1:]))


def tiny_forward(layers, x):
    """layers: the 9 file entries; x [3][size][size] RGB in [0, 1] -> [B * (5 + C)][S][S]"""
    assert len(layers) == N_LAYERS
    for l in range(8):
        x = conv_layer(x, layers[l])
        if l < 5:
            x = maxpool_chw(x)
        elif l == 5:
            x = maxpool_s1_chw(x)
    return conv_layer(x, layers[8], leaky=False)


def _conv(x, W):
    """x [N][H][W][C], W [k][k][c][n] -> [N][H][W][n]: stride 1, zero padding k / 2"""
    y = F.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), padding=W.shape[0] // 2)
    return y.permute(0, 2, 3, 1)


def _pool(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


def _pool_s1(x):
    padded = F.pad(x.permute(0, 3, 1, 2), (0, 1, 0, 1), value=-float("inf"))
    return F.max_pool2d(padded, 2, 1).permute(0, 2, 3, 1)


class Pass:
    """one forward pass in training mode and, after backward(cotangent), every gradient the device test reads"""

    def __init__(self, layers, x):
        assert len(layers) == N_LAYERS
        t = lambda a: torch.tensor(np.ascontiguousarray(np.asarray(a, np.float64)), dtype=torch.float64, requires_grad=True)
        self.W = [t(np.asarray(d["weights"]).transpose(2, 3, 1, 0)) for d in layers]
        self.gamma = [t(d["scales"]) for d in layers[:8]]
        self.beta = [t(d["biases"]) for d in layers[:8]]
        self.b_last = t(layers[8]["biases"])
        self.batch_var, self.count = [None] * 8, [0] * 8
        h = torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
        for l in range(6):
            h = self._layer(h, l)
            if l < 5:
                h = _pool(h)
        self.fine = h
        self.fine.retain_grad()
        self.cat = _pool_s1(self.fine)                       # the head's input: what the device keeps as last_dcat
        self.cat.retain_grad()
        h = self._layer(self._layer(self.cat, 6), 7)
        self.out = _conv(h, self.W[8]) + self.b_last

    def _layer(self, x, l):
        y = _conv(x, self.W[l])
        mean = y.mean(dim=(0, 1, 2))
        var = ((y - mean) ** 2).mean(dim=(0, 1, 2))                     # biased, as Darknet normalises
        self.batch_var[l] = var.detach().numpy().copy()
        self.count[l] = y.shape[0] * y.shape[1] * y.shape[2]
        z = (y - mean) / torch.sqrt(var + EPS) * self.gamma[l] + self.beta[l]
        return torch.where(z > 0, z, 0.1 * z)

    def backward(self, cotangent):
        self.out.backward(torch.as_tensor(np.asarray(cotangent, np.float64)).reshape(self.out.shape))
        g = lambda t: t.grad.numpy()
        self.dW = [g(w) for w in self.W]
        self.dgamma, self.dbeta = [g(v) for v in self.gamma], [g(v) for v in self.beta]
        self.db_last, self.dcat, self.dfine = g(self.b_last), g(self.cat), g(self.fine)
        return self
