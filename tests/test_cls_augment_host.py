"""The classifier's augmentation specification (img_dataset/augment_cls.py) and its host batcher (img_dataset/
cls_images.py) on the host: the warp against expected arrays worked out here, the draws, the order.  Everything is
equality.  No GPU."""
import os

import numpy as np
import pytest


def _AC():
    from tensorflow_yolo2_amd.img_dataset import augment_cls
    return augment_cls


def _img(h, w, seed=0):
    return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def write_list(tmp_path, shapes, seed=5):
    """PNG files of random pixels (lossless: the decoded bytes are the arrays) -> ([(path, label)], [BGR arrays])"""
    from PIL import Image
    items, imgs = [], []
    for k, (h, w) in enumerate(shapes):
        bgr = _img(h, w, seed + k)
        path = os.path.join(str(tmp_path), "im%02d.png" % k)
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path)
        items.append((path, (7 * k + 3) % 1000))
        imgs.append(bgr)
    return items, imgs


# ---- warp_affine_u8
def test_integer_translation_is_the_exact_crop():
    AC = _AC()
    img = _img(20, 30)
    out = AC.warp_affine_u8(img, [1, 0, 5, 0, 1, -3], 12, 16, 99)
    want = np.full((12, 16, 3), 99, np.uint8)
    want[3:, :] = img[0:9, 5:21]                       # rows -3 .. -1 lie above the image
    assert (out == want).all()
    out = AC.warp_affine_u8(img, [1, 0, 22, 0, 1, 15], 12, 16, 0)
    want = np.zeros((12, 16, 3), np.uint8)
    want[:5, :8] = img[15:20, 22:30]                   # beyond the right and the bottom edge
    assert (out == want).all()


def test_mirror_matrix_returns_the_mirrored_image():
    AC = _AC()
    img = _img(9, 14)
    assert (AC.warp_affine_u8(img, [-1, 0, 13, 0, 1, 0], 9, 14, 7) == img[:, ::-1]).all()
    row = AC.compose(9, 14, 14, 9, 0, 0, 0.0, True)
    assert (AC.warp_affine_u8(img, row, 9, 14, 7) == img[:, ::-1]).all()


@pytest.mark.parametrize("N", [8, 34])
def test_quarter_turns_equal_rot90_about_the_integer_centre(N):
    """inverse rotation about (N // 2, N // 2) = (N / 2, N / 2): out[v, u] = img[u, N - v] at 90 degrees, img[N - v, N - u]
    at 180, img[N - u, v] at 270 -- np.rot90 (counter-clockwise) shifted by the one row / column that leaves the image"""
    AC = _AC()
    img = _img(N, N)
    fill = 201
    want = {}
    want[90] = np.full_like(img, fill)
    want[90][1:, :] = np.rot90(img, 1)[:-1, :]
    want[180] = np.full_like(img, fill)
    want[180][1:, 1:] = np.rot90(img, 2)[:-1, :-1]
    want[270] = np.full_like(img, fill)
    want[270][:, 1:] = np.rot90(img, 3)[:, :-1]
    for v in range(N):                                 # the index form of the docstring, on a few pixels
        for u in (0, 1, N - 1):
            if v >= 1:
                assert (want[90][v, u] == img[u, N - v]).all()
            if u >= 1:
                assert (want[270][v, u] == img[N - u, v]).all()
    for deg in (90, 180, 270):
        M = AC.compose(N, N, N, N, 0, 0, float(deg), False)
        assert (AC.warp_affine_u8(img, M, N, N, fill) == want[deg]).all(), deg
    assert (AC.warp_affine_u8(img, AC.compose(N, N, N, N, 0, 0, 0.0, False), N, N, fill) == img).all()
    assert (AC.warp_affine_u8(img, AC.compose(N, N, N, N, 0, 0, -90.0, False), N, N, fill) == want[270]).all()
    assert (AC.warp_affine_u8(img, AC.compose(N, N, N, N, 0, 0, 360.0, False), N, N, fill) == img).all()


def test_coordinates_that_are_no_coordinates_give_fill():
    AC = _AC()
    img = _img(6, 6)
    for bad in (float("nan"), float("inf"), -float("inf")):            # anywhere: inf * 0 is no number either
        for k in range(6):
            M = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            M[k] = bad
            assert (AC.warp_affine_u8(img, M, 6, 8, 33) == 33).all(), (bad, k)
    for bad in (2.0 ** 31, -2.0 ** 31, 2.0 ** 30, -2.0 ** 30):
        for k in (2, 5):
            M = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
            M[k] = bad
            assert (AC.warp_affine_u8(img, M, 6, 8, 33) == 33).all(), (bad, k)
    # a huge factor: the pixels it multiplies by 0 stay coordinates
    out = AC.warp_affine_u8(img, [2.0 ** 29, 0, 0, 0, 1, 0], 6, 8, 33)
    assert (out[:, 0] == img[:, 0]).all() and (out[:, 1] == img[:, 0] * 0 + 33).all() and (out[:, 2:] == 33).all()


def test_constant_image_stays_constant_inside_and_fill_outside():
    AC = _AC()
    img = np.full((40, 50, 3), (10, 200, 77), np.uint8)
    for deg in (0.0, 7.0, 33.3, 45.0, 123.4, 180.0, -61.0):
        M = AC.compose(40, 50, 64, 48, 3, 1, deg, deg > 40)
        out = AC.warp_affine_u8(img, M, 32, 32, 10).astype(np.int64)
        sx, sy = AC.source_coords(M, 32, 32)
        inside = (sx >= 0) & (sx <= 49) & (sy >= 0) & (sy <= 39)        # all four taps that weigh are image pixels
        outside = (sx < -1) | (sx >= 50) | (sy < -1) | (sy >= 40)
        assert inside.any() and (out[inside] == (10, 200, 77)).all(), deg
        assert (out[outside] == 10).all()
        assert (out[..., 0] == 10).all()               # channel 0 equals the fill: constant everywhere, border blends too


# ---- draw_batch
def test_draw_batch_consumes_one_block_whatever_the_branches():
    AC = _AC()
    a, b = AC.generator(3, 0), AC.generator(3, 0)
    AC.ClsAugment(crop_chance=0.0, flip=False).draw_batch(a, [(500, 375)] * 6, 224)
    AC.ClsAugment(crop_chance=1.0, angle=180).draw_batch(b, [(10, 10), (1, 1), (300, 700), (64, 64), (5, 900), (2, 3)], 64)
    assert a.bit_generator.state == b.bit_generator.state
    c = AC.generator(3, 0)
    c.random((6, AC.NDRAW))
    assert a.bit_generator.state == c.bit_generator.state
    AC.ClsAugment().skip(c, 6, 2)
    a.random((12, AC.NDRAW))
    assert a.bit_generator.state == c.bit_generator.state


def test_every_crop_window_lies_inside_its_scaled_image():
    AC = _AC()
    rng = np.random.default_rng(11)
    aug = AC.ClsAugment(angle=180)
    hs = np.concatenate([[1, 1, 2, 31, 32, 33], rng.integers(1, 700, 1994)])
    ws = np.concatenate([[1, 2, 1, 33, 32, 31], rng.integers(1, 700, 1994)])
    shapes = np.stack([hs, ws], axis=1)
    for size in (32, 224):
        u = rng.random((len(shapes), AC.NDRAW))
        u[:8, AC.D_OFFX] = u[:8, AC.D_OFFY] = u[:8, AC.D_SIDE] = 1.0 - 2.0 ** -53     # the top of every range
        g = aug.geometry(u, shapes, size)
        for k in ("scaled_w", "scaled_h", "off_x", "off_y"):
            assert (g[k] == np.floor(g[k])).all(), k
        assert (g["off_x"] >= 0).all() and (g["off_x"] + size <= g["scaled_w"]).all()
        assert (g["off_y"] >= 0).all() and (g["off_y"] + size <= g["scaled_h"]).all()
        hi = int(np.floor(size * aug.crop_ratio))
        short = np.where(g["W"] > g["H"], g["scaled_h"], g["scaled_w"])
        assert (short[g["crop"]] >= size).all() and (short[g["crop"]] <= hi).all()
        assert (short[g["crop"]] == hi).any() and g["crop"].any() and (~g["crop"]).any()
        assert ((g["scaled_w"] == size) & (g["scaled_h"] == size))[~g["crop"]].all()
        assert (np.abs(g["deg"]) <= 180).all()
    assert int(np.floor(224 * aug.crop_ratio)) == 292


def test_too_small_takes_the_stretch_branch():
    """int(long * (L / short)) can fall below `size` when the short side is drawn at `size` itself and the quotient
    rounds down; the geometry then is the stretch, whatever the crop coin says"""
    AC = _AC()
    aug = AC.ClsAugment(crop_chance=1.0)
    found = 0
    for n in range(1, 400):                            # square images: long = short, long * (size / short) may be size - ulp
        u = np.zeros((1, AC.NDRAW))                    # L = size, crop coin passes
        g = aug.geometry(u, [(n, n)], 224)
        longer = np.floor(np.float64(n) * (np.float64(224) / np.float64(n)))
        if longer < 224:
            found += 1
            assert not g["crop"][0] and g["scaled_w"][0] == 224 and g["scaled_h"][0] == 224
            assert g["off_x"][0] == 0 and g["off_y"][0] == 0
        else:
            assert g["crop"][0]
    assert found > 0


def test_flip_off_changes_no_other_column():
    AC = _AC()
    shapes = [(375, 500), (500, 375), (64, 64), (100, 30)] * 4
    on = AC.ClsAugment(flip=True).draw_batch(AC.generator(1, 0), shapes, 224)
    off = AC.ClsAugment(flip=False).draw_batch(AC.generator(1, 0), shapes, 224)
    u = AC.generator(1, 0).random((16, AC.NDRAW))
    mirrored = u[:, AC.D_MIRROR] >= 0.5
    assert mirrored.any() and (~mirrored).any()
    assert (on[~mirrored] == off[~mirrored]).all()
    assert (on[:, 3:] == off[:, 3:]).all()             # the y row of the map and the colour triple
    W = np.array([s[1] for s in shapes], np.float64)[mirrored]
    assert (on[mirrored, 0] == -off[mirrored, 0]).all() and (on[mirrored, 1] == -off[mirrored, 1]).all()
    assert (on[mirrored, 2] == (W - 1.0) - off[mirrored, 2]).all()


def test_rows_depend_on_seed_and_rank_alone():
    AC = _AC()
    shapes = [(375, 500), (500, 375), (64, 64)]
    aug = AC.ClsAugment()
    a = aug.draw_batch(AC.generator(4, 1), shapes, 224)
    assert (a == aug.draw_batch(AC.generator(4, 1), shapes, 224)).all()
    assert (a != aug.draw_batch(AC.generator(4, 0), shapes, 224)).any()
    assert (a != aug.draw_batch(AC.generator(5, 1), shapes, 224)).any()
    assert a.shape == (3, AC.ROW) and a.dtype == np.float64
    assert (a[:, 6:] == a[:, 6:].astype(np.float32)).all()              # the colour triple holds float32 values
    # the colour columns as Augment.draw forms them, from the same uniforms
    u = AC.generator(4, 1).random((3, AC.NDRAW))
    s = 1.0 + 0.5 * u[:, AC.D_SAT]
    assert (a[:, AC.SAT] == np.float32(np.where(u[:, AC.D_SATINV] >= 0.5, 1.0 / s, s))).all()
    assert (np.abs(a[:, AC.HUE]) <= 0.1).all()


def test_identity_row_of_an_image_of_the_output_size_returns_it():
    AC = _AC()
    for n in (32, 64, 33):
        img = _img(n, n)
        row = AC.identity_row(n, n, n)
        assert (row == [1, 0, 0, 0, 1, 0, 0, 1, 1]).all()
        assert (AC.ClsAugment().image(img, row, n) == img).all()
        assert (AC.plain_image(img, n) == img).all()


def test_arguments_are_refused_with_the_field_named():
    AC = _AC()
    for field, bad in (("angle", -1), ("angle", 181), ("crop_chance", 1.5), ("crop_ratio", 0.9), ("hue", 0.6),
                       ("saturation", 0.5), ("exposure", 0.9), ("fill", 256), ("fill", 1.5)):
        with pytest.raises(ValueError, match=field):
            AC.ClsAugment(**{field: bad})


def test_tile_path_names_the_three_paths():
    AC = _AC()
    big = AC.identity_row(300, 260, 32)                # scale above 8: the box of one tile is the whole image
    assert AC.tile_path(300, 260, 784, 0, big, 32, 32, 0, 0) == "inplace"
    crop = np.array([1, 0, 3, 0, 1, -5, 0, 1, 1], np.float64)
    assert AC.tile_path(48, 64, 192, 0, crop, 64, 64, 0, 0) == "staged"
    away = np.array([1, 0, 1000, 0, 1, 0, 0, 1, 1], np.float64)
    assert AC.tile_path(48, 64, 192, 0, away, 64, 64, 0, 0) == "fill"
    nan = np.array([float("nan"), 0, 0, 0, 1, 0, 0, 1, 1], np.float64)
    assert AC.tile_path(48, 64, 192, 0, nan, 64, 64, 0, 0) == "inplace"
    assert AC.tile_path(48, 64, 193, 1, crop, 64, 64, 0, 0) == "inplace"     # an unaligned pool cannot be staged


# ---- cls_images
SHAPES = [(40, 52), (64, 48), (33, 33), (90, 70), (37, 53), (50, 120), (32, 32)]


def test_cls_images_is_deterministic_and_matches_the_specification(tmp_path):
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    AC = _AC()
    items, imgs = write_list(tmp_path, SHAPES)
    aug = AC.ClsAugment(angle=30)
    a, b = cls_images(items, 5, seed=2, augment=aug), cls_images(items, 5, seed=2, augment=aug)
    for _ in range(3):                                 # crosses the wrap of 7 images at batch 5
        ia, la = a.get_u8(32)
        ib, lb = b.get_u8(32)
        assert (ia == ib).all() and (la == lb).all() and ia.dtype == np.uint8 and la.dtype == np.int32
    c = cls_images(items, 5, seed=3, augment=aug)
    assert (c.get_u8(32)[0] != cls_images(items, 5, seed=2, augment=aug).get_u8(32)[0]).any()
    # the first batch by hand: the order, one block of draws, image by image
    d = cls_images(items, 5, seed=2, augment=aug)
    order = [g['entry'] for g in d.gt_labels[:5]]
    rows = aug.draw_batch(AC.generator(2, 0), [SHAPES[e] for e in order], 64)
    got, labels = d.get_u8(64)
    for k, e in enumerate(order):
        assert (got[k] == aug.image(imgs[e], rows[k], 64)).all()
        assert labels[k] == items[e][1]
    # augmenting changes no batch order
    p, q = cls_images(items, 5, seed=2), cls_images(items, 5, seed=2, augment=aug)
    for _ in range(3):
        assert (p.get_u8(32)[1] == q.get_u8(32)[1]).all()
    assert (cls_images(items, 5, seed=2).get_u8(32)[0][0] == AC.plain_image(imgs[order[0]], 32)).all()


def test_rank_sharding_partitions_an_epoch(tmp_path):
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    items, _ = write_list(tmp_path, [(32, 32)] * 6)
    label_to_entry = {l: k for k, (_, l) in enumerate(items)}
    for world in (1, 2, 3):
        seen = []
        for rank in range(world):
            b = cls_images(items, 6 // world, seed=9, rank=rank, world=world)
            seen += [label_to_entry[int(l)] for l in b.get_u8(32)[1]]
        assert sorted(seen) == list(range(6)), (world, seen)


def test_skip_batches_equals_drawing_them(tmp_path):
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    AC = _AC()
    items, _ = write_list(tmp_path, SHAPES)
    for aug in (None, AC.ClsAugment(angle=180)):
        a, b = cls_images(items, 5, seed=1, augment=aug), cls_images(items, 5, seed=1, augment=aug)
        for _ in range(3):
            a.get_u8(32)
        b.skip_batches(3)
        ia, la = a.get_u8(64)
        ib, lb = b.get_u8(64)
        assert (ia == ib).all() and (la == lb).all()


def test_pool_short_side_stores_the_resized_shape(tmp_path):
    from tensorflow_yolo2_amd.img_dataset import cls_images as CI
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import resize_bilinear_u8
    items, imgs = write_list(tmp_path, [(90, 70), (50, 120), (40, 40), (33, 64)])
    b = CI.cls_images(items, 2, pool_short_side=40)
    assert b.shapes.tolist() == [[int(90 * (40.0 / 70)), 40], [40, int(120 * (40.0 / 50))], [40, 40], [33, 64]]
    assert (b.images[0] == resize_bilinear_u8(imgs[0], 51, 40)).all()
    assert (b.images[2] == imgs[2]).all() and (b.images[3] == imgs[3]).all()
    assert CI.stored_shape(500, 375, 292) == (389, 292) and CI.stored_shape(375, 500, None) == (375, 500)
    with pytest.raises(ValueError, match="pool_short_side"):
        CI.cls_images(items, 2, pool_short_side=0)
