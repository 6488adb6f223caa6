"""The evaluation views of a classifier image, as a host specification (numpy only): each view is one parameter row of
augment_cls.py -- an affine map through augment_cls.compose and the colour triple (0, 1, 1), for which y2_warp_u8_batch
skips its colour stage -- so the device batch of DeviceCls.eval_views equals view_images bit for bit.  Nothing here is new
arithmetic.

  "stretch"  1 view: augment_cls.identity_row, the image stretched to size x size
  "centre"   1 view, Darknet's validate_classifier_single: the short side scaled to L = size, the long side to
             int(long * (L / short)) in the float64 operations of ClsAugment's crop branch, the centre size x size crop at
             off = (scaled - size) // 2; angle 0, no mirror
  "ten"      10 views, Darknet's validate_classifier_10: L = size + margin; the crops at top-left (0, 0), top-right
             (scaled_w - size, 0), bottom-left, bottom-right and the centre, then the same five mirrored

What differs from Darknet: it stretches the image to (w + 32)^2 before its ten crops and lets the
corner offsets leave the image; here the aspect ratio is kept and every crop lies inside the scaled image."""
import numpy as np

from .augment_cls import ROW, compose, warp_affine_u8

VIEWS = {"stretch": 1, "centre": 1, "ten": 10}


def _scaled(H, W, L):
    """(scaled_w, scaled_h) float64 arrays: the short side L, the long side int(long * (L / short)) -- ClsAugment.geometry's
    crop branch (ties: the width is the short side).  The long side is not let below L: for a square image the rounded
    product long * (L / short) can be L - 1 ulp (49 * (32 / 49) < 32), which ClsAugment answers by its stretch branch
    and which here would put a crop offset at -1."""
    wide = W > H
    factor = L / np.where(wide, H, W)
    longer = np.maximum(np.floor(np.where(wide, W, H) * factor), L)     # int() of a positive number
    return np.where(wide, longer, L), np.where(wide, L, longer)


def view_rows(shapes, size, views, margin=32):
    """shapes [n][2] = (height, width) -> float64 [n, V, ROW]: the parameter rows of every image's views"""
    if views not in VIEWS:
        raise ValueError("views %r is not one of %s" % (views, ", ".join(sorted(VIEWS))))
    if int(size) != size or size < 32 or size % 32:
        raise ValueError("size %r is not a positive multiple of 32" % (size,))
    if margin < 0:
        raise ValueError("margin %r below 0" % (margin,))
    shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
    if (shapes < 1).any():
        raise ValueError("a shape with a side below 1")
    size = int(size)
    H, W = shapes[:, 0].astype(np.float64), shapes[:, 1].astype(np.float64)
    out = np.empty((len(shapes), VIEWS[views], ROW), np.float64)
    out[:, :, 6:] = (0.0, 1.0, 1.0)
    if views == "stretch":                                      # identity_row of every shape, as one vector expression
        out[:, 0, :6] = compose(H, W, float(size), float(size), 0, 0, 0.0, False)
        return out
    L = float(size) if views == "centre" else float(size) + float(margin)
    sw, sh = _scaled(H, W, L)
    fx, fy = sw - size, sh - size                               # the far offsets; >= 0 because both sides are >= L
    cx, cy = np.floor(fx / 2.0), np.floor(fy / 2.0)
    zero = np.zeros_like(fx)
    offsets = [(cx, cy)] if views == "centre" else [(zero, zero), (fx, zero), (zero, fy), (fx, fy), (cx, cy)]
    mirrors = (False,) if views == "centre" else (False, True)
    v = 0
    for mirror in mirrors:
        for ox, oy in offsets:
            out[:, v, :6] = compose(H, W, sw, sh, ox, oy, 0.0, mirror)
            v += 1
    return out


def view_images(img, rows, size, fill=127):
    """[H, W, 3] uint8 and its rows [V, ROW] -> uint8 [V, size, size, 3]: the host reference of DeviceCls.eval_views"""
    rows = np.asarray(rows, np.float64).reshape(-1, ROW)
    return np.stack([warp_affine_u8(img, r[:6], size, size, fill) for r in rows])
