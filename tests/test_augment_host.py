"""The augmentation specification (img_dataset/augment.py) on the host: against a slow scalar restatement written here
(Python loops over np.float32 scalars, the window cut by explicit index tests), its properties, the label rule, the
draws, the batch order and the argument checks.  Everything is equality except the one test that says otherwise.
No GPU."""
import os

import numpy as np
import pytest

from test_device_voc_host import make_devkit

F = np.float32


def _A():
    from tensorflow_yolo2_amd.img_dataset import augment
    return augment


# ---- the restatement: one pixel / one output sample at a time
def _slow_pixel(b8, g8, r8, hue, sat, exp):
    hue, sat, exp = F(hue), F(sat), F(exp)
    if hue == F(0) and sat == F(1) and exp == F(1):
        return int(b8), int(g8), int(r8)
    b, g, r = F(b8) / F(255), F(g8) / F(255), F(r8) / F(255)
    v = max(max(r, g), b)
    d = F(v - min(min(r, g), b))
    s = F(0) if v == F(0) else F(d / v)
    if d == F(0):
        h = F(0)
    elif v == r:
        h = F(F(g - b) / d)
    elif v == g:
        h = F(F(2) + F(F(b - r) / d))
    else:
        h = F(F(4) + F(F(r - g) / d))
    h = F(h + F(F(6) * hue))
    if h < F(0):
        h = F(h + F(6))
    if h >= F(6):
        h = F(h - F(6))
    s = min(F(s * sat), F(1))
    v = min(F(v * exp), F(1))
    i = F(np.floor(h))
    f = F(h - i)
    p = F(v * F(F(1) - s))
    q = F(v * F(F(1) - F(s * f)))
    t = F(v * F(F(1) - F(s * F(F(1) - f))))
    r2, g2, b2 = {0: (v, t, p), 1: (q, v, p), 2: (p, v, t), 3: (p, q, v), 4: (t, p, v), 5: (v, p, q)}[int(i)]
    return tuple(min(max(int(F(F(x * F(255)) + F(0.5))), 0), 255) for x in (b2, g2, r2))


def _slow_distort(img, hue, sat, exp):
    out = np.empty_like(img)
    flat_in, flat_out = img.reshape(-1, 3), out.reshape(-1, 3)
    for k in range(len(flat_in)):
        flat_out[k] = _slow_pixel(flat_in[k, 0], flat_in[k, 1], flat_in[k, 2], hue, sat, exp)
    return out


def _slow_axis(o, n_in, n_out):
    f = (o + 0.5) * (n_in / n_out) - 0.5
    i0 = int(np.floor(f))
    frac = 0.0 if i0 < 0 else f - i0
    w1 = int(np.rint(frac * 2048))
    return min(max(i0, 0), n_in - 1), min(max(i0 + 1, 0), n_in - 1), w1


def _slow_crop_resize(img, row, out_h, out_w, fill, flip=False):
    im_h, im_w = img.shape[:2]
    x0, y0, cw, ch = (int(v) for v in row[:4])

    def window(y, x, c):
        sy, sx = y0 + y, x0 + x
        return int(img[sy, sx, c]) if 0 <= sy < im_h and 0 <= sx < im_w else fill

    out = np.empty((out_h, out_w, 3), np.uint8)
    mirror = bool(flip) != bool(row[4])
    for oy in range(out_h):
        ya, yb, wy1 = _slow_axis(oy, ch, out_h)
        for ox in range(out_w):
            xa, xb, wx1 = _slow_axis(out_w - 1 - ox if mirror else ox, cw, out_w)
            for c in range(3):
                top = window(ya, xa, c) * (2048 - wx1) + window(ya, xb, c) * wx1
                bot = window(yb, xa, c) * (2048 - wx1) + window(yb, xb, c) * wx1
                out[oy, ox, c] = (top * (2048 - wy1) + bot * wy1 + (1 << 21)) >> 22
    return out


TRIPLES = ((0.1, 1.5, 1.5), (-0.1, 1 / 1.5, 1 / 1.5), (0.5, 1.0, 1.0), (-0.5, 3.0, 0.25), (0.0, 1.0, 1.3), (0.0, 0.7, 1.0),
           (0.03125, 1.0, 1.0), (0.0, 1.0, 1.0), (0.3337, 8.0, 4.0))


def test_distort_equals_the_scalar_restatement():
    A = _A()
    rng = np.random.default_rng(5)
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).reshape(16, 16, 3)
    primaries = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255],
                          [0, 0, 0], [255, 255, 255], [1, 0, 0], [0, 0, 1], [254, 255, 255], [128, 128, 127]],
                         np.uint8).reshape(3, 4, 3)
    images = [gray, primaries] + [rng.integers(0, 256, (7, 9, 3), dtype=np.uint8) for _ in range(3)]
    for (hue, sat, exp) in TRIPLES:
        for img in images:
            got = A.distort_hsv_u8(img, hue, sat, exp)
            assert got.dtype == np.uint8 and got.shape == img.shape
            assert np.array_equal(got, _slow_distort(img, hue, sat, exp)), (hue, sat, exp)


def test_crop_resize_equals_the_scalar_restatement():
    A = _A()
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (11, 14, 3), dtype=np.uint8)
    windows = {"inside": (3, 2, 8, 6), "whole": (0, 0, 14, 11), "left": (-4, 1, 9, 8), "right": (7, 2, 12, 7),
               "top": (2, -5, 9, 10), "bottom": (1, 6, 10, 9), "all four": (-3, -2, 21, 16), "one pixel": (5, 5, 1, 1),
               "outside": (20, 3, 4, 4), "corner": (-2, -2, 3, 3)}
    for name, (x0, y0, cw, ch) in windows.items():
        for (oh, ow) in ((8, 12), (13, 5), (32, 32)):
            for rflip in (0, 1):
                row = np.array([x0, y0, cw, ch, rflip, 0, 1, 1], np.float64)
                for tflip in (False, True):
                    got = A.crop_resize_u8(img, row, oh, ow, 127, tflip)
                    assert np.array_equal(got, _slow_crop_resize(img, row, oh, ow, 127, tflip)), (name, oh, ow, rflip, tflip)
    # the two mirrors cancel
    row = np.array([-3, -2, 21, 16, 1, 0, 1, 1], np.float64)
    plain = np.array([-3, -2, 21, 16, 0, 0, 1, 1], np.float64)
    assert np.array_equal(A.crop_resize_u8(img, row, 8, 12, 9, True), A.crop_resize_u8(img, plain, 8, 12, 9, False))


def _fixtures(golden_dir):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import imread_bgr, parse_annotation
    imgs = [imread_bgr(os.path.join(golden_dir, n)) for n in ("testImg1.jpg", "testImg2.jpg")]
    objs, shape = parse_annotation(os.path.join(golden_dir, "testImg2Anno.xml"))
    assert shape == imgs[1].shape[:2] == (500, 353) and len(objs) >= 2
    return imgs, objs


def test_identity_row_is_the_plain_resize_and_encoder(golden_dir):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import encode_boxes, flip_label, resize_bilinear_u8
    A = _A()
    imgs, objs = _fixtures(golden_dir)
    aug = A.Augment()
    for img in imgs:
        h, w = img.shape[:2]
        for (oh, ow) in ((416, 416), (64, 64), (97, 150)):
            want = resize_bilinear_u8(img, oh, ow)
            assert np.array_equal(aug.image(img, A.identity_row(h, w), oh, ow), want)
            assert np.array_equal(aug.image(img, A.identity_row(h, w, 1), oh, ow), want[:, ::-1])
            assert np.array_equal(aug.image(img, A.identity_row(h, w), oh, ow, flip=True), want[:, ::-1])
    for size, S in ((224, 7), (416, 13), (608, 19)):
        want = encode_boxes(objs, 500, 353, size, S)
        assert np.array_equal(A.encode_boxes_window(objs, A.identity_row(500, 353), size, S), want)
        assert np.array_equal(A.encode_boxes_window(objs, A.identity_row(500, 353), size, S, flip=True), flip_label(want, size))
        assert np.array_equal(A.encode_boxes_window(objs, A.identity_row(500, 353, 1), size, S), flip_label(want, size))


def test_colour_properties():
    A = _A()
    rng = np.random.default_rng(8)
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1).reshape(16, 16, 3)
    for hue in (-0.5, -0.1, 0.0, 0.07, 0.5):
        for sat in (1 / 3.0, 1.0, 1.5, 10.0):
            assert np.array_equal(A.distort_hsv_u8(gray, hue, sat, 1.0), gray)       # no hue, no saturation to change
    img = rng.integers(0, 256, (20, 20, 3), dtype=np.uint8)
    for exp in (0.5, 1 / 1.5, 1.25, 1.5, 4.0):
        got = A.distort_hsv_u8(img, 0.0, 1.0, exp).max(axis=-1)
        v = np.minimum((img.max(axis=-1).astype(F) / F(255)) * F(exp), F(1))
        assert np.array_equal(got, (v * F(255) + F(0.5)).astype(np.int32))
        if exp >= 4:
            assert (got[img.max(axis=-1) >= 64] == 255).all()                        # saturates
    # half a turn twice is a whole turn: back at the start within one level (an INEQUALITY, the only one in this file:
    # the intermediate image is rounded to uint8)
    for hue in (0.5, -0.5):
        back = A.distort_hsv_u8(A.distort_hsv_u8(img, hue, 1.0, 1.0), hue, 1.0, 1.0)
        assert np.abs(back.astype(int) - img.astype(int)).max() <= 1
    assert not np.array_equal(A.distort_hsv_u8(img, 0.5, 1.0, 1.0), img)


def test_overhang_is_the_distorted_fill(golden_dir):
    A = _A()
    imgs, _ = _fixtures(golden_dir)
    img = imgs[0]                                                                     # 240 x 352
    aug = A.Augment(fill=127)
    row = np.array([-176, -120, 704, 480, 0, 0.1, 1.5, 1 / 1.5], np.float64)         # the image in the middle half
    out = aug.image(img, row, 64, 64)
    fill = A.distort_hsv_u8(np.full((1, 1, 3), 127, np.uint8), 0.1, 1.5, 1 / 1.5)[0, 0]
    frame = np.ones((64, 64), bool)
    frame[15:49, 15:49] = False                                                       # output samples that touch the image
    assert (out[frame] == fill).all() and not (out[~frame] == fill).all()
    other = A.Augment(fill=3).image(img, row, 64, 64)
    assert (other[frame] == A.distort_hsv_u8(np.full((1, 1, 3), 3, np.uint8), 0.1, 1.5, 1 / 1.5)[0, 0]).all()
    assert np.array_equal(other[20:44, 20:44], out[20:44, 20:44])                     # the inside does not see the fill


def test_labels_follow_the_window():
    A = _A()
    objs = [(101.0, 51.0, 201.0, 151.0, 3), (301.0, 201.0, 341.0, 241.0, 7)]        # centres (150, 100) and (320, 220), 0-based
    size, S = 416, 13
    row = np.array([50, 20, 208, 208, 0, 0, 1, 1], np.float64)                       # columns 50..257, rows 20..227
    lab = A.encode_boxes_window(objs, row, size, S)
    assert lab[:, :, 0].sum() == 1                                                    # the second centre (320, 220) left it
    cy, cx = np.argwhere(lab[:, :, 0] == 1)[0]
    sx = size / 208
    want = [((200 - 50) * sx + (100 - 50) * sx) / 2.0, ((150 - 20) * sx + (50 - 20) * sx) / 2.0,
            (200 - 50) * sx - (100 - 50) * sx, (150 - 20) * sx - (50 - 20) * sx]
    assert lab[cy, cx, 1:5].tolist() == want and (cx, cy) == (int(want[0] * S / size), int(want[1] * S / size))
    assert lab[cy, cx, 5 + 3] == 1 and lab[cy, cx, 5:].sum() == 1
    # a box that overhangs the window is clamped, and its cell comes from the clamped centre
    row = np.array([120, 0, 200, 400, 0, 0, 1, 1], np.float64)
    lab = A.encode_boxes_window(objs[:1], row, size, S)
    x1, x2 = max((100 - 120) * (size / 200), 0), (200 - 120) * (size / 200)
    assert x1 == 0 and lab[:, :, 0].sum() == 1 and lab[lab[:, :, 0] == 1][0, 1] == (x2 + x1) / 2.0
    # the mirror is flip_label's
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import flip_label
    frow = row.copy()
    frow[4] = 1
    assert np.array_equal(A.encode_boxes_window(objs, frow, size, S), flip_label(A.encode_boxes_window(objs, row, size, S), size))
    assert np.array_equal(A.encode_boxes_window(objs, frow, size, S, flip=True), A.encode_boxes_window(objs, row, size, S))


LABEL_SEED, LABEL_DRAWS = 3, 64
LABEL_JITTER = 0.45                                     # at 0.3 neither centre of this annotation can leave the window
LABEL_KEPT, LABEL_DROPPED = 111, 17                     # computed once from the rule restated in the test


def test_kept_and_dropped_objects_over_seeded_draws(golden_dir):
    """64 windows drawn with seed 3 on testImg2Anno.xml: which objects stay, and in which cells, is restated here from
    the rule (unclamped centre inside the window), and the totals are pinned.  The annotation's two centres, (121, 305)
    and (179, 254) in a 353 x 500 image, are further than 0.3 of the image from every edge, so the draws use jitter
    0.45: a set of draws that drops nothing would not test the rule."""
    A = _A()
    _, objs = _fixtures(golden_dir)
    aug, rng = A.Augment(jitter=LABEL_JITTER), A.generator(LABEL_SEED, 0)
    size, S = 416, 13
    kept = dropped = 0
    for _ in range(LABEL_DRAWS):
        row = aug.draw(rng, 500, 353)
        sx, sy = size / row[2], size / row[3]
        cells = set()
        for (xmin, ymin, xmax, ymax, _c) in objs:
            ux = ((xmax - 1 - row[0]) * sx + (xmin - 1 - row[0]) * sx) / 2.0
            uy = ((ymax - 1 - row[1]) * sy + (ymin - 1 - row[1]) * sy) / 2.0
            if 0 <= ux < size and 0 <= uy < size:
                kept += 1
                x1, x2 = (min(max((v - 1 - row[0]) * sx, 0), size - 1) for v in (xmin, xmax))
                y1, y2 = (min(max((v - 1 - row[1]) * sy, 0), size - 1) for v in (ymin, ymax))
                cx, cy = int((x2 + x1) / 2.0 * S / size), int((y2 + y1) / 2.0 * S / size)
                cells.add((cy, S - 1 - cx if row[4] else cx))
            else:
                dropped += 1
        lab = A.encode_boxes_window(objs, row, size, S)
        assert {tuple(c) for c in np.argwhere(lab[:, :, 0] == 1).tolist()} == cells
    assert kept + dropped == LABEL_DRAWS * len(objs)
    assert (kept, dropped) == (LABEL_KEPT, LABEL_DROPPED)


def test_draws():
    A = _A()
    aug = A.Augment()
    a = [aug.draw(A.generator(4, 0), 333, 500) for _ in range(2)]
    assert np.array_equal(a[0], a[1])                                                # a seed, a stream
    r0, r1, s5 = A.generator(4, 0), A.generator(4, 1), A.generator(5, 0)
    rows0 = np.array([aug.draw(r0, 333, 500) for _ in range(200)])
    rows1 = np.array([aug.draw(r1, 333, 500) for _ in range(200)])
    assert not np.array_equal(rows0, rows1) and not np.array_equal(rows0[0], aug.draw(s5, 333, 500))
    for rows in (rows0, rows1):
        assert rows.dtype == np.float64 and rows.shape == (200, 8)
        assert (rows[:, :5] == np.rint(rows[:, :5])).all() and set(rows[:, 4]) == {0.0, 1.0}
        assert (rows[:, 2] >= 1).all() and (rows[:, 3] >= 1).all()
        assert (rows[:, 0] >= -0.3 * 500).all() and (rows[:, 0] + rows[:, 2] <= 1.3 * 500 + 1).all()
        assert (rows[:, 1] >= -0.3 * 333 - 1).all() and (rows[:, 1] + rows[:, 3] <= 1.3 * 333 + 1).all()
        assert (np.abs(rows[:, 5]) <= F(0.1)).all()
        for col in (6, 7):
            assert (rows[:, col] >= F(1 / 1.5)).all() and (rows[:, col] <= F(1.5)).all()
            assert (rows[:, col] < 1).any() and (rows[:, col] > 1).any()
        assert (rows[:, 5:] == rows[:, 5:].astype(np.float32)).all()                 # float32 values
        assert rows[:, 0].min() < 0 < rows[:, 0].max() and rows[:, 2].min() < 500 < rows[:, 2].max()
    # flip=False consumes the coin: the other columns are those of flip=True
    off = np.array([A.Augment(flip=False).draw(A.generator(4, 0), 333, 500)])
    assert off[0, 4] == 0 and np.array_equal(np.delete(off[0], 4), np.delete(a[0], 4))
    calm = A.Augment(jitter=0, hue=0, saturation=1, exposure=1, flip=False).draw(A.generator(1, 0), 333, 500)
    assert np.array_equal(calm, A.identity_row(333, 500))


def test_augmenting_does_not_change_the_batch_order(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    A = _A()
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=3)             # 4 images, 8 entries
    for rank, world in ((0, 1), (1, 2)):
        kw = dict(batch_size=2, devkit_path=kit, image_size=64, flipped=True, seed=9, rank=rank, world=world)
        plain, aug = pascal_voc("trainval", **kw), pascal_voc("trainval", augment=A.Augment(), **kw)
        assert not hasattr(plain, "aug_rng")                                         # augment=None creates no generator
        for _ in range(2 * plain.per_rank // 2):                                     # two epochs
            for ds in (plain, aug):
                images, labels = ds.get_u8()
                assert images.shape == (2, 64, 64, 3) and images.dtype == np.uint8 and labels.shape == (2, 2, 2, 25)
            assert plain.cursor == aug.cursor
        seq = [[(g["imname"], g["flipped"]) for g in ds.gt_labels] for ds in (plain, aug)]
        assert seq[0] == seq[1]                                                      # same list after the same reshuffles
    # the images themselves, entry by entry over two epochs
    kw = dict(batch_size=1, devkit_path=kit, image_size=64, flipped=True, seed=9)
    plain, aug = pascal_voc("trainval", **kw), pascal_voc("trainval", augment=A.Augment(), **kw)
    order = [[], []]
    for k, ds in enumerate((plain, aug)):
        real_next = ds._next

        def spy(real_next=real_next, k=k):
            g = real_next()
            order[k].append((g["imname"], g["flipped"]))
            return g
        ds._next = spy
        for _ in range(16):
            ds.get_u8()
    assert order[0] == order[1] and len(order[0]) == 16 and len(set(order[0])) == 8
    a, b = pascal_voc("trainval", augment=A.Augment(), **kw), pascal_voc("trainval", augment=A.Augment(), **kw)
    first = [a.get_u8() for _ in range(3)]
    for (ia, la), (ib, lb) in zip(first, [b.get_u8() for _ in range(3)]):
        assert np.array_equal(ia, ib) and np.array_equal(la, lb)                     # deterministic
    f32, _ = pascal_voc("trainval", augment=A.Augment(), **kw).get()
    assert f32.dtype == np.float32 and np.array_equal(f32, (first[0][0].astype(np.float32) / 255.0) * 2.0 - 1.0)


def test_validation():
    A = _A()
    for bad in (dict(jitter=-0.1), dict(jitter=0.5), dict(hue=-0.01), dict(hue=0.51), dict(saturation=0.9),
                dict(exposure=0.5), dict(fill=-1), dict(fill=256), dict(fill=1.5), dict(jitter=float("nan"))):
        with pytest.raises(ValueError):
            A.Augment(**bad)
    a = A.Augment()
    assert (a.jitter, a.hue, a.saturation, a.exposure, a.flip, a.fill) == (0.3, 0.1, 1.5, 1.5, True, 127)
    A.Augment(jitter=0, hue=0.5, saturation=1, exposure=1, fill=0)
    from tensorflow_yolo2_amd.pascal import pascal_train_darknet as P
    for bad in (["--augment"], ["--augment", "--multi-scale"], ["--augment", "--devkit", "x", "--jitter", "0.5"],
                ["--augment", "--devkit", "x", "--saturation", "0.5"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    args = P.parse_args(["--augment", "--devkit", "x"])
    assert repr(args.augmentation) == repr(A.Augment()) and not args.device_data
    assert P.parse_args(["--augment", "--devkit", "x", "--multi-scale"]).device_data
    assert P.parse_args(["--devkit", "x"]).augmentation is None
    got = P.parse_args(["--augment", "--devkit", "x", "--jitter", "0.2", "--hue", "0.05", "--saturation", "2", "--exposure", "1.25"])
    assert repr(got.augmentation) == repr(A.Augment(0.2, 0.05, 2.0, 1.25))
