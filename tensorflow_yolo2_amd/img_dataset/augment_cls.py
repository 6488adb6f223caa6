"""Training augmentation of the classifier batches, as a host specification (numpy only): a coin-flip mirror, a rotation
about the image centre, a random short-side scale with a random square crop (or, one time in four, a plain stretch) and
the hue / saturation / exposure distortion of img_dataset/augment.py.  Modelled on image_read(data_aug=True) of the
reference's ILSVRC loader (img_dataset/ilsvrc2017_cls_multithread.py:320-415) and on Darknet's classifier recipe (angle,
hue, saturation, exposure, random scale and crop).  The arithmetic below is this repository's own specification -- no
byte of cv2's output is pinned -- and the kernel of csrc/augment.hip (y2_warp_u8_batch) equals it bit for bit.

One sample's augmentation is a parameter row of 9 doubles {m00, m01, m02, m10, m11, m12, hue, sat, exp}:
  m00 .. m12      the affine map from an OUTPUT pixel index (u, v) to a SOURCE pixel coordinate:
                  sx = (m00 * u + m01 * v) + m02, sy = (m10 * u + m11 * v) + m12, every product and sum rounded on its
                  own in float64.  The whole geometry -- mirror, rotation, scale, crop -- is this one map, so a pixel is
                  interpolated ONCE (the reference interpolates in warpAffine and again in resize).
  hue, sat, exp   float32 values, as in augment.py: (0, 1, 1) is no distortion.

What differs from the reference is listed in DESIGN.md section 9: one bilinear tap through the composed map, 11-bit
weights (cv2's warp tables have 5 bits), a fill of 127 (fill=0 is the reference's black border), Darknet's 7 degrees by
default (angle=180 is the reference's full turn, as a real number), and the colour stage of augment.py in place of the
reference's additive uint8 H / S shifts and gamma curve."""
import math

import numpy as np

from .augment import distort_hsv_u8

ROW = 9                                     # doubles per parameter row
M00, M01, M02, M10, M11, M12, HUE, SAT, EXP = range(ROW)
STREAM = 0xC15                              # last word of the augmentation generator's seed sequence
# columns of the one rng.random((B, NDRAW)) block of a batch; every column is consumed whatever the branches taken
NDRAW = 11
D_MIRROR, D_ANGLE, D_CROP, D_SIDE, D_OFFX, D_OFFY, D_HUE, D_SAT, D_SATINV, D_EXP, D_EXPINV = range(NDRAW)
LIMIT = float(1 << 30)                      # a source coordinate of this magnitude (or not finite) reads as fill

# the kernel's geometry (csrc/augment.hip: kWarpTile, kWarpLds), restated for tile_path
TILE = 32
LDS_BUDGET = 32768

_f32 = np.float32


def generator(seed, rank):
    """the augmentation stream of one rank: its own generator, so that augmenting changes no batch order"""
    return np.random.default_rng([int(seed), int(rank), STREAM])


def source_coords(M, out_h, out_w):
    """(sx, sy) float64 [out_h, out_w] of every output pixel, in the specification's operation order"""
    m = [np.float64(x) for x in np.asarray(M, np.float64).reshape(6)]
    u = np.arange(out_w, dtype=np.float64)[None, :]
    v = np.arange(out_h, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        sx = (m[0] * u + m[1] * v) + m[2]
        sy = (m[3] * u + m[4] * v) + m[5]
    return sx, sy


def warp_affine_u8(img_bgr_u8, M, out_h, out_w, fill):
    """[H, W, 3] uint8 -> [out_h, out_w, 3] uint8 through the map M (six float64: output index -> source coordinate).
    A coordinate that is not finite or of magnitude >= 2^30 makes the pixel `fill` (decided before any conversion to
    integer).  Otherwise x0 = floor(sx), wx = (int)((sx - x0) * 2048 + 0.5) in 0 .. 2048, y0 / wy likewise; the taps
    (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) read `fill` outside [0, W) x [0, H); per channel in int32
    top = p00 * (2048 - wx) + p01 * wx, bot likewise, (top * (2048 - wy) + bot * wy + 2^21) >> 22: the blend of
    csrc/augment.hip's resize_pixel, below 2^31.  A weight of 0 or 2048 returns a source byte."""
    img = np.asarray(img_bgr_u8)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3, (img.dtype, img.shape)
    if not (0 <= int(fill) <= 255 and int(fill) == fill):
        raise ValueError("fill %r is not an integer of 0..255" % (fill,))
    H, W = img.shape[:2]
    sx, sy = source_coords(M, out_h, out_w)
    with np.errstate(all="ignore"):
        valid = (np.abs(sx) < LIMIT) & (np.abs(sy) < LIMIT)      # False for a NaN and for an infinity
    sx, sy = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
    fx, fy = np.floor(sx), np.floor(sy)
    wx = ((sx - fx) * 2048.0 + 0.5).astype(np.int64)[..., None]
    wy = ((sy - fy) * 2048.0 + 0.5).astype(np.int64)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    a = img.astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        p = a[np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)]
        return np.where(inside[..., None], p, int(fill))

    top = tap(x0, y0) * (2048 - wx) + tap(x0 + 1, y0) * wx
    bot = tap(x0, y0 + 1) * (2048 - wx) + tap(x0 + 1, y0 + 1) * wx
    out = (top * (2048 - wy) + bot * wy + (1 << 21)) >> 22
    return np.where(valid[..., None], out, int(fill)).astype(np.uint8)


def rotation(deg):
    """(alpha, beta) = (cos, sin) of the angle in degrees, float64 arrays.  A quarter turn is decided, not left to
    rounding: a multiple of 90 takes alpha, beta of {0, +-1} exactly."""
    deg = np.asarray(deg, np.float64)
    rad = deg * (math.pi / 180.0)                               # math.radians
    alpha, beta = np.cos(rad), np.sin(rad)
    q = deg / 90.0
    quarter = q == np.floor(q)
    k = np.where(quarter, np.mod(q, 4.0), 0.0).astype(np.int64)
    alpha = np.where(quarter, np.array([1.0, 0.0, -1.0, 0.0])[k], alpha)
    beta = np.where(quarter, np.array([0.0, 1.0, 0.0, -1.0])[k], beta)
    return alpha, beta


def compose(H, W, scaled_w, scaled_h, off_x, off_y, deg, mirror):
    """[..., 6] float64: the map of an output pixel (u, v) to the source, as the reference orders its steps (mirror,
    rotate on the source canvas, then scale and crop), composed in this fixed order of float64 operations:
      scaled index -> canvas   xs = u + off_x, xr = (xs + 0.5) * (W / scaled_w) - 0.5 = ax * u + bx with
                               ax = W / scaled_w, bx = (off_x + 0.5) * ax - 0.5; ay, by likewise (pixel centres)
      inverse rotation         about (cx, cy) = (W // 2, H // 2), cv2's sign (positive is counter-clockwise, origin top
                               left): src_x = alpha * (xr - cx) - beta * (yr - cy) + cx,
                               src_y = beta * (xr - cx) + alpha * (yr - cy) + cy, that is
                               m00 = alpha * ax, m01 = -(beta * ay), m02 = (alpha * (bx - cx) - beta * (by - cy)) + cx
                               m10 = beta * ax,  m11 = alpha * ay,   m12 = (beta * (bx - cx) + alpha * (by - cy)) + cy
      mirror                   src_x <- W - 1 - src_x: m00 = -m00, m01 = -m01, m02 = (W - 1) - m02"""
    H, W = np.asarray(H, np.float64), np.asarray(W, np.float64)
    alpha, beta = rotation(deg)
    ax, ay = W / np.asarray(scaled_w, np.float64), H / np.asarray(scaled_h, np.float64)
    bx = (np.asarray(off_x, np.float64) + 0.5) * ax - 0.5
    by = (np.asarray(off_y, np.float64) + 0.5) * ay - 0.5
    cx, cy = np.floor(W / 2.0), np.floor(H / 2.0)
    dx, dy = bx - cx, by - cy
    m00, m01, m02 = alpha * ax, -(beta * ay), (alpha * dx - beta * dy) + cx
    m10, m11, m12 = beta * ax, alpha * ay, (beta * dx + alpha * dy) + cy
    mirror = np.asarray(mirror, bool)
    m00, m01, m02 = np.where(mirror, -m00, m00), np.where(mirror, -m01, m01), np.where(mirror, (W - 1.0) - m02, m02)
    return np.stack(np.broadcast_arrays(m00, m01, m02, m10, m11, m12), axis=-1)


def identity_row(H, W, size):
    """the row of the plain path: the stretch branch with no mirror, angle 0 and the colour triple (0, 1, 1).  What
    y2_warp_u8_batch forms itself from the table row when it is given no parameters."""
    row = np.empty(ROW, np.float64)
    row[:6] = compose(H, W, size, size, 0, 0, 0.0, False)
    row[6:] = (0.0, 1.0, 1.0)
    return row


def _int_between(u, lo, hi):
    """an integer of [lo, hi] from a uniform u of [0, 1): lo + min(floor(u * (hi - lo + 1)), hi - lo), as float64"""
    span = hi - lo
    return lo + np.minimum(np.floor(u * (span + 1.0)), span)


class ClsAugment(object):
    def __init__(self, angle=7.0, crop_chance=0.75, crop_ratio=292.0 / 224.0, hue=0.1, saturation=1.5, exposure=1.5,
                 flip=True, fill=127):
        if not 0 <= angle <= 180:
            raise ValueError("angle %r outside [0, 180]" % (angle,))
        if not 0 <= crop_chance <= 1:
            raise ValueError("crop_chance %r outside [0, 1]" % (crop_chance,))
        if not 1 <= crop_ratio <= 16:
            raise ValueError("crop_ratio %r outside [1, 16]" % (crop_ratio,))
        if not 0 <= hue <= 0.5:
            raise ValueError("hue %r outside [0, 0.5]" % (hue,))
        if not saturation >= 1:
            raise ValueError("saturation %r below 1" % (saturation,))
        if not exposure >= 1:
            raise ValueError("exposure %r below 1" % (exposure,))
        if not (0 <= fill <= 255 and int(fill) == fill):
            raise ValueError("fill %r is not an integer of 0..255" % (fill,))
        self.angle, self.crop_chance, self.crop_ratio = float(angle), float(crop_chance), float(crop_ratio)
        self.hue, self.saturation, self.exposure = float(hue), float(saturation), float(exposure)
        self.flip, self.fill = bool(flip), int(fill)

    def __repr__(self):
        return ("ClsAugment(angle=%r, crop_chance=%r, crop_ratio=%r, hue=%r, saturation=%r, exposure=%r, flip=%r, "
                "fill=%r)" % (self.angle, self.crop_chance, self.crop_ratio, self.hue, self.saturation, self.exposure,
                              self.flip, self.fill))

    def geometry(self, u, shapes, size):
        """the per-sample quantities of a block u [B, NDRAW] of uniforms for images of shapes [B][2] = (height, width):
        a dict of arrays -- mirror (bool), deg, crop (bool: the crop branch was taken), scaled_w, scaled_h, off_x, off_y
        (float64 holding integers).  Crop branch, as the reference (:378-403): the short side becomes L, an integer of
        [size, floor(size * crop_ratio)], the long side int(long * (L / short)); when a scaled side falls below `size`
        (its "too small") or the crop coin fails, the stretch branch: scaled to size x size, offsets 0."""
        u = np.asarray(u, np.float64)
        shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
        assert u.shape == (len(shapes), NDRAW), (u.shape, shapes.shape)
        assert (shapes >= 1).all(), "an image without pixels"
        size = int(size)
        H, W = shapes[:, 0].astype(np.float64), shapes[:, 1].astype(np.float64)
        mirror = (u[:, D_MIRROR] >= 0.5) & self.flip            # the coin is consumed also when flip is off
        deg = self.angle * (2.0 * u[:, D_ANGLE] - 1.0)
        crop = u[:, D_CROP] < self.crop_chance
        L = _int_between(u[:, D_SIDE], float(size), float(math.floor(size * self.crop_ratio)))
        wide = W > H                                            # else the width is the short side (ties: the width)
        factor = L / np.where(wide, H, W)
        longer = np.floor(np.where(wide, W, H) * factor)        # int() of a positive number
        scaled_w, scaled_h = np.where(wide, longer, L), np.where(wide, L, longer)
        crop = crop & (scaled_w >= size) & (scaled_h >= size)
        scaled_w, scaled_h = np.where(crop, scaled_w, float(size)), np.where(crop, scaled_h, float(size))
        off_x = _int_between(u[:, D_OFFX], 0.0, scaled_w - size)
        off_y = _int_between(u[:, D_OFFY], 0.0, scaled_h - size)
        return {"H": H, "W": W, "mirror": mirror, "deg": deg, "crop": crop, "scaled_w": scaled_w, "scaled_h": scaled_h,
                "off_x": off_x, "off_y": off_y}

    def colour(self, u):
        """[B, 3] float64 holding the float32 triple hue, sat, exp, formed as Augment.draw forms it: hue ~ U(-hue, hue);
        sat and exp ~ U(1, max), inverted on a coin"""
        hue = _f32(-self.hue + (2.0 * self.hue) * u[:, D_HUE])
        s = 1.0 + (self.saturation - 1.0) * u[:, D_SAT]
        e = 1.0 + (self.exposure - 1.0) * u[:, D_EXP]
        sat = _f32(np.where(u[:, D_SATINV] >= 0.5, 1.0 / s, s))
        exp = _f32(np.where(u[:, D_EXPINV] >= 0.5, 1.0 / e, e))
        return np.stack([hue, sat, exp], axis=1).astype(np.float64)

    def rows(self, u, shapes, size):
        """[B, ROW] float64 of a block of uniforms: vector arithmetic, no per-sample Python"""
        g = self.geometry(u, shapes, size)
        out = np.empty((len(g["H"]), ROW), np.float64)
        out[:, :6] = compose(g["H"], g["W"], g["scaled_w"], g["scaled_h"], g["off_x"], g["off_y"], g["deg"],
                             g["mirror"])
        out[:, 6:] = self.colour(np.asarray(u, np.float64))
        return out

    def draw_batch(self, rng, shapes, size):
        """the parameter rows of one batch: exactly ONE rng.random((B, NDRAW)) block, whatever the branches taken"""
        shapes = np.asarray(shapes, np.int64).reshape(-1, 2)
        return self.rows(rng.random((len(shapes), NDRAW)), shapes, size)

    def skip(self, rng, batch_size, batches):
        """advance the stream by whole batches of `batch_size` samples"""
        for _ in range(int(batches)):
            rng.random((int(batch_size), NDRAW))

    def image(self, img, row, size):
        """the augmented uint8 BGR image of one sample: one warp, then the colour stage (fill pixels included)"""
        out = warp_affine_u8(img, row[:6], size, size, self.fill)
        return distort_hsv_u8(out, row[HUE], row[SAT], row[EXP])


def plain_image(img, size, fill=127):
    """the image of the plain path (augment=None): identity_row through the same warp, no colour stage"""
    img = np.asarray(img)
    return warp_affine_u8(img, identity_row(img.shape[0], img.shape[1], size)[:6], size, size, fill)


def tile_path(H, W, pitch, offset, row, out_h, out_w, tile_x, tile_y):
    """"fill", "staged" or "inplace": the path the kernel takes for the TILE x TILE output tile (tile_x, tile_y) of a
    sample with parameter row `row` on a table row {offset, H, W, pitch}.  The restatement of warp_u8_kernel's rule:
    the source box of the tile is spanned by its four corners through M (the map is monotone in u and in v, rounding
    included), one pixel more to the right and below for the second tap, cut to the image.  A corner that is not a
    valid coordinate -> the taps read the pool in place (every pixel tests itself); an empty box -> the tile is fill;
    the 16-byte aligned row segments of the box within LDS_BUDGET bytes -> staged in LDS; else in place."""
    m = [np.float64(x) for x in np.asarray(row, np.float64)[:6]]
    u0, v0 = TILE * tile_x, TILE * tile_y
    u1, v1 = min(u0 + TILE - 1, out_w - 1), min(v0 + TILE - 1, out_h - 1)
    xs, ys = [], []
    with np.errstate(all="ignore"):
        for (u, v) in ((u0, v0), (u1, v0), (u0, v1), (u1, v1)):
            u, v = np.float64(u), np.float64(v)
            xs.append((m[0] * u + m[1] * v) + m[2])
            ys.append((m[3] * u + m[4] * v) + m[5])
        if not all(abs(c) < LIMIT for c in xs + ys):
            return "inplace"
    bx0, bx1 = max(int(math.floor(min(xs))), 0), min(int(math.floor(max(xs))) + 1, W - 1)
    by0, by1 = max(int(math.floor(min(ys))), 0), min(int(math.floor(max(ys))) + 1, H - 1)
    if bx0 > bx1 or by0 > by1:
        return "fill"
    if (offset | pitch) & 15 or pitch < 3 * W:
        return "inplace"
    a0, a1 = (3 * bx0) & ~15, (3 * bx1 + 3 + 15) & ~15
    return "staged" if (a1 - a0) * (by1 - by0 + 1) <= LDS_BUDGET else "inplace"
