"""The TRAINING pass of yolov2-voc.cfg in torch float64 autograd on the CPU, written from Darknet's arithmetic on the
arrays of a `.weights` file (utils/darknet_weights.split), NHWC like the device:

    convolutional   conv with zero padding k / 2, then with batch_normalize=1 the BATCH statistics of the map -- mean and
                    biased variance over N, H, W, (x - mean) / sqrt(var + .000001) * scales + biases --, leaky .1; the
                    last layer is conv + biases, linear
    maxpool         size 2, stride 2
    reorg           the index table of utils/darknet_reorg.reorg_darknet_table
    route           layers=-1,-4: the reorganised map, then the 13x13 path

Darknet's 1x1 fourth layer runs here as this repository runs it: 3x3 with the file's filter on the centre tap, the same
function under zero padding, so the gradient of all nine taps can be compared.

Test helper only: the gradients of the device's train graph are compared with what autograd gives for this."""
import numpy as np
import torch
import torch.nn.functional as F

from tensorflow_yolo2_amd.utils.darknet_reorg import reorg_darknet_table

POOL_AFTER = (0, 1, 4, 7)
EPS = 1e-6
K_MODEL = {3: 3}                 # file layer -> the filter size this repository's graph runs it with


def _filters(d, l):
    """[n][c][k][k] -> [k][k][c][n] float64, the 1x1 fourth layer on the centre tap of a 3x3"""
    w = np.asarray(d["weights"], np.float64).transpose(2, 3, 1, 0)
    if K_MODEL.get(l, w.shape[0]) != w.shape[0]:
        big = np.zeros((3, 3) + w.shape[2:], np.float64)
        big[1, 1] = w[0, 0]
        w = big
    return torch.tensor(np.ascontiguousarray(w), dtype=torch.float64, requires_grad=True)


def _conv(x, W):
    """x [N][H][W][C], W [k][k][c][n] -> [N][H][W][n]: stride 1, zero padding k / 2"""
    k = W.shape[0]
    y = F.conv2d(x.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), padding=k // 2)
    return y.permute(0, 2, 3, 1)


def _pool(x):
    return F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)


class Pass:
    """one forward pass in training mode and, after backward(cotangent), every gradient the device test reads"""

    def __init__(self, layers, x):
        assert len(layers) == 23
        self.W = [_filters(d, l) for l, d in enumerate(layers)]
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)
        self.gamma = [t(d["scales"]) for d in layers[:22]]
        self.beta = [t(d["biases"]) for d in layers[:22]]
        self.b_last = t(layers[22]["biases"])
        self.batch_var, self.count = [None] * 22, [0] * 22
        h = torch.tensor(np.asarray(x, np.float64), dtype=torch.float64)
        for l in range(13):
            h = self._layer(h, l)
            if l in POOL_AFTER:
                h = _pool(h)
        self.fine = h
        self.fine.retain_grad()
        h = _pool(self.fine)
        for l in range(13, 20):
            h = self._layer(h, l)
        r = self._layer(self.fine, 20)
        js, is_, cs = (torch.as_tensor(a) for a in reorg_darknet_table(r.shape[1], r.shape[2], r.shape[3]))
        self.cat = torch.cat([r[:, js, is_, cs], h], dim=3)
        self.cat.retain_grad()
        h = self._layer(self.cat, 21)
        self.out = _conv(h, self.W[22]) + self.b_last

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
