"""Darknet's `reorg` layer (stride 2) as yolov2-voc.cfg runs it: the specification of y2_passthrough_concat_darknet.

It is NOT the space-to-depth of oracle/ext_ref.reorg.  Darknet's forward pass calls `reorg_cpu(..., forward = 0)` with the
INPUT's dimensions, whose index arithmetic treats the input [C][H][W] as [C/4][2H][2W]: each image's C*H*W values are
scrambled across channels AND positions, and no permutation of the next layer's filter channels reproduces it.  A
network trained by Darknet has learnt its filters behind exactly this scramble, so a reader of its `.weights` files has
to apply it.

`reorg_darknet_chw` is the loop form, as Darknet writes it; `reorg_darknet` is the same map per image in this
repository's NHWC through ONE vectorised index table (`reorg_darknet_table`).  tests/test_darknet_weights_host.py holds
the two equal element for element.

The map is a permutation of each image's values, so its gradient is the inverse permutation: `reorg_darknet_backward`
and `passthrough_concat_darknet_backward`, written from the same table, are the specification of
y2_passthrough_concat_darknet_backward (tests/test_darknet_train_host.py)."""
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


def reorg_darknet_backward(dout):
    """dout [N][H/2][W/2][4C] -> the gradient [N][H][W][C] of reorg_darknet's input.  The reorg is a permutation of each
    image's values (the table is a bijection), so its gradient is the inverse permutation: every row of the index table
    names the ONE input element an output element was read from, and that element receives the output's gradient.
    Written from the table as a scatter through unique indices -- the specification of the reorganised part of
    y2_passthrough_concat_darknet_backward."""
    dout = np.asarray(dout)
    n, Ho, Wo, C4 = dout.shape
    if C4 % 16:
        raise ValueError("reorg_darknet_backward: %d channels are not 4 C with C %% 4 == 0" % C4)
    H, W, C = 2 * Ho, 2 * Wo, C4 // 4
    js, is_, cs = reorg_darknet_table(H, W, C)
    flat = ((js * W + is_) * C + cs).reshape(-1)         # the input element of every output element, per image
    if np.unique(flat).size != H * W * C:
        raise AssertionError("reorg_darknet_table is no permutation at H %d, W %d, C %d" % (H, W, C))
    din = np.empty((n, H * W * C), dout.dtype)
    din[:, flat] = dout.reshape(n, -1)
    return din.reshape(n, H, W, C)


def passthrough_concat_darknet_backward(dout, cf):
    """dout [N][H][W][4 cf + Cc] -> (dfine [N][2H][2W][cf], dcoarse [N][H][W][Cc]): the split at channel 4 cf, the front
    part through reorg_darknet_backward"""
    dout = np.asarray(dout)
    if dout.ndim != 4 or cf < 4 or cf % 4 or dout.shape[3] <= 4 * cf:
        raise ValueError("passthrough_concat_darknet_backward: dout %s does not split at 4 * %d" % (dout.shape, cf))
    return reorg_darknet_backward(dout[..., :4 * cf]), np.ascontiguousarray(dout[..., 4 * cf:])
