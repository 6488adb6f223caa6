"""Darknet's `reorg` layer (stride 2) as yolov2-voc.cfg runs it: the specification of y2_passthrough_concat_darknet.

It is NOT the space-to-depth of oracle/ext_ref.reorg.  Darknet's forward pass calls `reorg_cpu(..., forward = 0)` with the
INPUT's dimensions, whose index arithmetic treats the input [C][H][W] as [C/4][2H][2W]: each image's C*H*W values are
scrambled across channels AND positions, and no permutation of the next layer's filter channels reproduces it.  A
network trained by Darknet has learnt its filters behind exactly this scramble, so a reader of its `.weights` files has
to apply it.

`reorg_darknet_chw` is the loop form, as Darknet writes it; `reorg_darknet` is the same map per image in this
repository's NHWC through ONE vectorised index table (`reorg_darknet_table`).  tests/test_darknet_weights_host.py holds
the two equal element for element."""
import numpy as np


def reorg_darknet_chw(x):
    """x [C][H][W] -> [4C][H/2][W/2]: reorg_cpu(x, W, H, C, batch 1, stride 2, forward 0, out), its four loops"""
    x = np.asarray(x)
    C, H, W = x.shape
    if C % 4 or H % 2 or W % 2:
        raise ValueError("reorg_darknet_chw: [%d][%d][%d] needs C %% 4 == 0 and even H, W" % (C, H, W))
    out_c = C // 4
    flat = x.reshape(-1)
    out = np.empty(C * H * W, x.dtype)
    for k in range(C):
        for j in range(H):
            for i in range(W):
                c2 = k % out_c
                off = k // out_c
                w2 = 2 * i + off % 2
                h2 = 2 * j + off // 2
                out[i + W * (j + H * k)] = flat[w2 + 2 * W * (h2 + 2 * H * c2)]
    return out.reshape(4 * C, H // 2, W // 2)


def reorg_darknet_table(H, W, C):
    """(js, is, cs), three int64 arrays [H/2][W/2][4C]: out[n, jo, io, co] = fine[n, js, is, cs] for fine [N][H][W][C]"""
    if C % 4 or H % 2 or W % 2 or min(H, W, C) < 1:
        raise ValueError("reorg_darknet_table: H %d, W %d, C %d needs C %% 4 == 0 and even H, W" % (H, W, C))
    Ho, Wo, out_c = H // 2, W // 2, C // 4
    jo, io, co = np.meshgrid(np.arange(Ho, dtype=np.int64), np.arange(Wo, dtype=np.int64),
                             np.arange(4 * C, dtype=np.int64), indexing="ij")
    q = io + Wo * (jo + Ho * co)                 # the output element in Darknet's [4C][Ho][Wo]
    i, j, k = q % W, (q // W) % H, q // (W * H)  # ... which its loops reach as (k, j, i) over [C][H][W]
    c2, off = k % out_c, k // out_c
    p = (2 * i + off % 2) + 2 * W * ((2 * j + off // 2) + 2 * H * c2)
    return (p // W) % H, p % W, p // (W * H)     # the input element in Darknet's [C][H][W]


def reorg_darknet(fine):
    """fine [N][H][W][C] -> [N][H/2][W/2][4C], Darknet's reorg of every image"""
    fine = np.asarray(fine)
    _n, H, W, C = fine.shape
    js, is_, cs = reorg_darknet_table(H, W, C)
    return fine[:, js, is_, cs]


def passthrough_concat_darknet(fine, coarse):
    """route layers=-1,-4 of yolov2-voc.cfg: the reorganised fine map in channels 0 .. 4 Cf - 1, coarse behind it"""
    return np.concatenate([reorg_darknet(fine), np.asarray(coarse)], axis=-1)
