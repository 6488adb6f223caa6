"""Darknet's `[maxpool] size=2 stride=1` (the sixth pool of tiny-yolo-voc.cfg): the specification of y2_maxpool2x2s1 and
y2_maxpool2x2s1_backward, in float32 on this repository's [N][H][W][C].

maxpool_layer.c runs it with padding = size - 1 = 1, so the output is H x W like the input, and with the window offset
-padding / 2, which is 0 in C: output (i, j) is the maximum over input (i + dy, j + dx), dy, dx in {0, 1}, of the taps
inside the map -- a window anchored top-left and clipped at the bottom and right edges.  The running maximum starts at
-FLT_MAX and is replaced on a strict `>`, taps in the order (0,0), (0,1), (1,0), (1,1): the first maximum wins a tie
(so -0.0 and +0.0 do not displace each other) and a NaN is never chosen.

The gradient sends every output's dy to its window's arg-max.  An input can be the arg-max of up to four windows; its
dx is the float32 sum, from +0, of their dy in ascending row-major order of the window anchors (i-1,j-1), (i-1,j),
(i,j-1), (i,j) -- the order in which Darknet's loop over the outputs adds them.

The one deliberate departure: a window that holds NaNs alone yields -FLT_MAX and routes no gradient, where Darknet's
arg-max of -1 would write out of bounds.

Both functions are loops over the four taps; everything else is elementwise numpy."""
import numpy as np

FLT_MAX = np.finfo(np.float32).max
TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (dy, dx) in Darknet's loop order: tap t = 2 dy + dx


def _pool(x):
    """-> (y float32 [N][H][W][C], tap int8 [N][H][W][C]: the winning tap of every window, -1 where none won)"""
    x = np.asarray(x)
    if x.ndim != 4 or x.dtype != np.float32 or min(x.shape) < 1:
        raise ValueError("maxpool_s1: x must be a non-empty float32 [N][H][W][C], not %s %s" % (x.dtype, x.shape))
    _n, H, W, _c = x.shape
    y = np.full(x.shape, -FLT_MAX, np.float32)
    tap = np.full(x.shape, -1, np.int8)
    for t, (dy, dx) in enumerate(TAPS):
        v = x[:, dy:, dx:]                       # tap t of the windows anchored at [:H - dy, :W - dx]; the rest clip it
        best, won = y[:, :H - dy, :W - dx], tap[:, :H - dy, :W - dx]
        with np.errstate(invalid="ignore"):
            greater = v > best                   # strict, and False for a NaN
        best[greater] = v[greater]
        won[greater] = t
    return y, tap


def maxpool_s1(x):
    """x float32 [N][H][W][C] -> y float32 [N][H][W][C]"""
    return _pool(x)[0]


def maxpool_s1_backward(x, dy):
    """x, dy float32 [N][H][W][C] -> dx float32 [N][H][W][C]"""
    dy = np.asarray(dy)
    _y, tap = _pool(x)
    if dy.shape != tap.shape or dy.dtype != np.float32:
        raise ValueError("maxpool_s1_backward: dy must be float32 %s, not %s %s" % (tap.shape, dy.dtype, dy.shape))
    _n, H, W, _c = tap.shape
    dx = np.zeros(tap.shape, np.float32)
    # input (i, j) is tap (ty, tx) of the window anchored at (i - ty, j - tx): ascending anchors are DESCENDING taps
    for t in (3, 2, 1, 0):
        ty, tx = TAPS[t]
        won = tap[:, :H - ty, :W - tx] == t
        dst = dx[:, ty:, tx:]
        np.add(dst, dy[:, :H - ty, :W - tx], out=dst, where=won)
    return dx
