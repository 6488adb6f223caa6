"""Darknet-style training augmentation of the VOC batches, as a host specification (numpy only): a random crop / pad
window of the source ("jitter"), a hue / saturation / exposure distortion and a coin-flip mirror, with the defaults of
Darknet's yolov2-voc.cfg (jitter=.3, hue=.1, saturation=1.5, exposure=1.5).  Not in the reference, which trains on the
plain images and their flipped copies only; the arithmetic below is this repository's own
specification, and the kernels of csrc/augment.hip (y2_augment_u8_batch, y2_encode_labels_window) equal it bit for bit,
as csrc/data.hip equals pascal_voc.resize_bilinear_u8 / encode_boxes.

One sample's augmentation is a parameter row of 8 doubles {x0, y0, cw, ch, flip, hue, sat, exp}:
  x0, y0, cw, ch  the window in integer source pixels: columns x0 .. x0 + cw - 1, rows y0 .. y0 + ch - 1.  It may extend
                  beyond the image on any side; what lies outside reads as `fill`.  The window is resized to the batch
                  size exactly as resize_bilinear_u8 resizes an image of cw x ch pixels.
  flip            1: mirror the output columns (on top of the mirror of a flipped table entry: the two cancel)
  hue, sat, exp   float32 values: hue shift in turns, factors on saturation and value.  (0, 1, 1) is no distortion.
Every float32 operation of distort_hsv_u8 is one correctly rounded IEEE operation (+ - * /, comparisons, floor and
selects), so numpy and a kernel compiled without fused multiply-adds give the same bits."""
import numpy as np

from .pascal_voc import flip_label, resize_bilinear_u8

ROW = 8                                     # doubles per parameter row
X0, Y0, CW, CH, FLIP, HUE, SAT, EXP = range(ROW)
STREAM = 0xA06                              # last word of the augmentation generator's seed sequence

_f32 = np.float32


def identity_row(im_h, im_w, flip=0):
    """the row that changes nothing: the whole image, no colour distortion"""
    return np.array([0, 0, im_w, im_h, flip, 0, 1, 1], np.float64)


def generator(seed, rank):
    """the augmentation stream of one rank: its own generator, so that augmenting changes no batch order"""
    return np.random.default_rng([int(seed), int(rank), STREAM])


class Augment(object):
    def __init__(self, jitter=0.3, hue=0.1, saturation=1.5, exposure=1.5, flip=True, fill=127):
        if not 0 <= jitter < 0.5:
            raise ValueError("jitter %r outside [0, 0.5)" % (jitter,))
        if not 0 <= hue <= 0.5:
            raise ValueError("hue %r outside [0, 0.5]" % (hue,))
        if not saturation >= 1:
            raise ValueError("saturation %r below 1" % (saturation,))
        if not exposure >= 1:
            raise ValueError("exposure %r below 1" % (exposure,))
        if not (0 <= fill <= 255 and int(fill) == fill):
            raise ValueError("fill %r is not an integer of 0..255" % (fill,))
        self.jitter, self.hue, self.saturation, self.exposure = float(jitter), float(hue), float(saturation), float(exposure)
        self.flip, self.fill = bool(flip), int(fill)

    def __repr__(self):
        return "Augment(jitter=%r, hue=%r, saturation=%r, exposure=%r, flip=%r, fill=%r)" % (
            self.jitter, self.hue, self.saturation, self.exposure, self.flip, self.fill)

    def draw(self, rng, im_h, im_w):
        """one parameter row for an image of im_h x im_w pixels; the draws come in a fixed order and number.  (Python's
        round() is rint: half to even.)  Ten scalar calls of the Generator per sample, on the host, inside get()."""
        uniform, coin = rng.uniform, rng.integers
        jw, jh = self.jitter * im_w, self.jitter * im_h
        pleft, pright = uniform(-jw, jw), uniform(-jw, jw)
        ptop, pbot = uniform(-jh, jh), uniform(-jh, jh)
        x0, y0 = float(round(pleft)), float(round(ptop))
        cw, ch = max(1.0, im_w - x0 - round(pright)), max(1.0, im_h - y0 - round(pbot))
        mirror = coin(0, 2)                                 # consumed whether or not the mirror is on
        flip = float(mirror) if self.flip else 0.0
        hue = _f32(uniform(-self.hue, self.hue))
        s = uniform(1.0, self.saturation)
        sat = _f32(1.0 / s if coin(0, 2) == 1 else s)
        e = uniform(1.0, self.exposure)
        exp = _f32(1.0 / e if coin(0, 2) == 1 else e)
        return np.array((x0, y0, cw, ch, flip, hue, sat, exp), np.float64)

    def image(self, img, row, out_h, out_w, flip=False):
        """the augmented uint8 BGR image of one sample: window, resize, mirror, colour"""
        return distort_hsv_u8(crop_resize_u8(img, row, out_h, out_w, self.fill, flip), row[HUE], row[SAT], row[EXP])

    def label(self, objs, row, image_size, cell_size, num_class=20, flip=False):
        return encode_boxes_window(objs, row, image_size, cell_size, num_class, flip)


def cut_window(img, row, fill):
    """window [ch, cw, 3] uint8 of the row, `fill` wherever it leaves the image"""
    img = np.asarray(img)
    im_h, im_w = img.shape[:2]
    x0, y0, cw, ch = (int(row[k]) for k in (X0, Y0, CW, CH))
    assert cw >= 1 and ch >= 1, (cw, ch)
    window = np.full((ch, cw, 3), fill, np.uint8)
    xa, xb = max(x0, 0), min(x0 + cw, im_w)
    ya, yb = max(y0, 0), min(y0 + ch, im_h)
    if xa < xb and ya < yb:
        window[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return window


def crop_resize_u8(img, row, out_h, out_w, fill, flip=False):
    """resize_bilinear_u8 of the row's window (its coefficients with n_in = cw / ch), the output columns mirrored when
    exactly one of `flip` (the entry's) and the row's flip is set"""
    out = resize_bilinear_u8(cut_window(img, row, fill), out_h, out_w)
    return out[:, ::-1, :] if bool(flip) != bool(row[FLIP]) else out


def distort_hsv_u8(bgr_u8, hue, sat, exp):
    """uint8 BGR pixels through HSV in float32: hue + 6 * hue (in sixths of a turn, wrapped), s * sat and v * exp (both
    cut at 1), back to uint8 with (int)(x * 255 + 0.5).  The triple (0, 1, 1) returns the input: identity is decided, not
    left to rounding."""
    bgr_u8 = np.asarray(bgr_u8)
    assert bgr_u8.dtype == np.uint8 and bgr_u8.shape[-1] == 3
    hue, sat, exp = _f32(hue), _f32(sat), _f32(exp)
    if hue == 0 and sat == 1 and exp == 1:
        return bgr_u8.copy()
    one, zero, six = _f32(1), _f32(0), _f32(6)
    f = bgr_u8.astype(np.float32) / _f32(255)
    b, g, r = f[..., 0], f[..., 1], f[..., 2]
    v = np.maximum(np.maximum(r, g), b)
    d = v - np.minimum(np.minimum(r, g), b)
    s = np.where(v == 0, zero, d / np.where(v == 0, one, v))
    dd = np.where(d == 0, one, d)
    h = np.where(v == r, (g - b) / dd, np.where(v == g, _f32(2) + (b - r) / dd, _f32(4) + (r - g) / dd))
    h = np.where(d == 0, zero, h)
    h = h + six * hue
    h = np.where(h < 0, h + six, h)
    h = np.where(h >= six, h - six, h)
    s = np.minimum(s * sat, one)
    v = np.minimum(v * exp, one)
    i = np.floor(h)
    fr = h - i
    p = v * (one - s)
    q = v * (one - s * fr)
    t = v * (one - s * (one - fr))
    r2 = np.where((i == 0) | (i >= 5), v, np.where(i == 1, q, np.where(i == 4, t, p)))
    g2 = np.where(i == 0, t, np.where((i == 1) | (i == 2), v, np.where(i == 3, q, p)))
    b2 = np.where(i == 2, t, np.where((i == 3) | (i == 4), v, np.where(i >= 5, q, p)))
    out = np.stack([b2, g2, r2], axis=-1).astype(np.float32)
    assert f.dtype == np.float32 and out.dtype == np.float32 and h.dtype == np.float32
    return np.clip((out * _f32(255) + _f32(0.5)).astype(np.int32), 0, 255).astype(np.uint8)


def _window_boxes(objs, row, image_size):
    """the window arithmetic of both label formats, in double: per object of `objs` whose unclamped centre lies inside
    [0, image_size) in x and y -- the others are dropped -- the clamped box as (cx, cy, w, h, class index), in annotation
    order.  x = (bx - 1 - x0) * (image_size / cw), y likewise."""
    for (_j, cx, cy, w, h, cls_ind) in _window_boxes_indexed(objs, row, image_size):
        yield cx, cy, w, h, cls_ind


def _window_boxes_indexed(objs, row, image_size):
    """_window_boxes with the annotation index j of every survivor in front"""
    x0, y0, cw, ch = (float(int(row[k])) for k in (X0, Y0, CW, CH))     # integers, as cut_window reads them
    w_ratio = image_size / cw
    h_ratio = image_size / ch
    for j, (xmin, ymin, xmax, ymax, cls_ind) in enumerate(objs):
        x1, y1 = (float(xmin) - 1 - x0) * w_ratio, (float(ymin) - 1 - y0) * h_ratio
        x2, y2 = (float(xmax) - 1 - x0) * w_ratio, (float(ymax) - 1 - y0) * h_ratio
        cx, cy = (x2 + x1) / 2.0, (y2 + y1) / 2.0
        if not (0 <= cx < image_size and 0 <= cy < image_size):
            continue
        x1, y1 = max(min(x1, image_size - 1), 0), max(min(y1, image_size - 1), 0)
        x2, y2 = max(min(x2, image_size - 1), 0), max(min(y2, image_size - 1), 0)
        yield j, (x2 + x1) / 2.0, (y2 + y1) / 2.0, x2 - x1, y2 - y1, int(cls_ind)


def encode_boxes_window(objs, row, image_size, cell_size, num_class=20, flip=False):
    """pascal_voc.encode_boxes with the boxes following the row's window: x = (bx - 1 - x0) * (image_size / cw), y
    likewise, in double.  An object whose unclamped centre lies outside [0, image_size) in x or y is dropped; the others
    are clamped, placed and mirrored as encode_boxes / flip_label do."""
    label = np.zeros((cell_size, cell_size, 5 + num_class))
    for (cx, cy, w, h, cls_ind) in _window_boxes(objs, row, image_size):
        x_ind = int(cx * cell_size / image_size)
        y_ind = int(cy * cell_size / image_size)
        if label[y_ind, x_ind, 0] == 1:
            continue
        label[y_ind, x_ind, 0] = 1
        label[y_ind, x_ind, 1:5] = (cx, cy, w, h)
        label[y_ind, x_ind, 5 + cls_ind] = 1
    return flip_label(label, image_size) if bool(flip) != bool(row[FLIP]) else label


MAX_BOXES = 30                              # rows of a box list by default: Darknet's max_boxes of the v2 region layer


def encode_box_list(objs, row, image_size, max_boxes=MAX_BOXES, flip=False):
    """The label of the anchor model that keeps EVERY object: (truth [max_boxes, 5] float32 = cx, cy, w, h in pixels of
    the resized input and the class index, number of rows used).  Per object it is encode_boxes_window's arithmetic in
    double -- the window transform, the drop rule on the unclamped centre, the clamp -- without the "cell already taken"
    rule; a mirrored sample stores image_size - 1 - cx as flip_label does.  Objects stay in annotation order, those beyond
    max_boxes are dropped in that order, the rows beyond the count are zeros.  One cast to float32 per stored value, so a
    row equals [1:5] of the grid cell the same object wins.  With identity_row(H, W) this is the plain path:
    (x - 1 - 0) * (size / W) is encode_boxes' (x - 1) * w_ratio."""
    if not 1 <= int(max_boxes) <= 1024:
        raise ValueError("max_boxes %r outside 1..1024" % (max_boxes,))
    mirror = bool(flip) != bool(row[FLIP])
    truth = np.zeros((int(max_boxes), 5), np.float32)
    count = 0
    for (cx, cy, w, h, cls_ind) in _window_boxes(objs, row, image_size):
        if count == max_boxes:
            break
        truth[count] = (image_size - 1 - cx if mirror else cx, cy, w, h, cls_ind)
        count += 1
    return truth, count


# ---- Darknet's shuffle-then-cut: which objects a crowded image keeps
KEY_STREAM = 0xB0C                          # last word of the key generator's seed sequence (STREAM's neighbour)


def key_generator(seed, rank):
    """the stream the draw's keys come from, one uint32 per sample: a generator of its own, so that turning the draw on
    moves neither the batch order nor the augmentation rows"""
    return np.random.default_rng([int(seed), int(rank), KEY_STREAM])


def draw_key(rng):
    """the next key of the stream: one call of the Generator per sample, whatever the sample holds"""
    return int(rng.integers(0, 1 << 32, dtype=np.uint64))


def box_rank(key, j):
    """the 32-bit hash of (key, annotation index j) that orders an image's objects for the draw.  32-bit integer
    operations only -- xor, shift, multiply modulo 2^32 -- so that numpy and a kernel agree on every bit:
        x = key ^ (j * 0x9E3779B9)
        x = x ^ (x >> 16);  x = x * 0x7FEB352D
        x = x ^ (x >> 15);  x = x * 0x846CA68B
        x = x ^ (x >> 16)
    every product modulo 2^32.  (The two multipliers and three shifts are the published `lowbias32` integer finaliser;
    the first line spreads neighbouring indices by the 32-bit golden ratio.)  key and j may be arrays: the result is
    uint32 of their broadcast shape."""
    m = np.uint64(0xFFFFFFFF)
    key, j = np.asarray(key, np.uint64) & m, np.asarray(j, np.uint64) & m
    x = key ^ ((j * np.uint64(0x9E3779B9)) & m)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & m
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & m
    x = x ^ (x >> np.uint64(16))
    return x.astype(np.uint32)


def encode_box_list_draw(objs, row, image_size, max_boxes=MAX_BOXES, key=0, flip=False):
    """encode_box_list with Darknet's shuffle-then-cut in place of "the first max_boxes": (truth [max_boxes, 5] float32,
    number of rows used).  The survivors are exactly _window_boxes' survivors, each with its annotation index j and
    box_rank(key, j); the max_boxes survivors with the smallest (hash, j) are kept and written IN ANNOTATION ORDER, in
    encode_box_list's arithmetic.  So with at most max_boxes survivors the result is encode_box_list's bit for bit,
    whatever the key; with more it is exactly max_boxes of the uncut list's rows, and the key decides which.  `key` is
    one uint32 per sample (key_generator).  The specification of y2_encode_box_list_draw (csrc/augment.hip)."""
    if not 1 <= int(max_boxes) <= 1024:
        raise ValueError("max_boxes %r outside 1..1024" % (max_boxes,))
    if not 0 <= int(key) < 1 << 32:
        raise ValueError("key %r is no uint32" % (key,))
    mirror = bool(flip) != bool(row[FLIP])
    survivors = list(_window_boxes_indexed(objs, row, image_size))
    if len(survivors) > max_boxes:
        ranks = box_rank(int(key), [s[0] for s in survivors])
        first = sorted(range(len(survivors)), key=lambda k: (int(ranks[k]), survivors[k][0]))[:int(max_boxes)]
        survivors = [survivors[k] for k in sorted(first)]
    truth = np.zeros((int(max_boxes), 5), np.float32)
    for count, (_j, cx, cy, w, h, cls_ind) in enumerate(survivors):
        truth[count] = (image_size - 1 - cx if mirror else cx, cy, w, h, cls_ind)
    return truth, len(survivors)
