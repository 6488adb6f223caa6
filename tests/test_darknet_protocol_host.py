"""Darknet's test-time protocol on the host (no GPU): pascal_voc.letterbox_darknet against a loop-by-loop restatement of
Darknet's resize_image / letterbox_image, its fixed points and its last-row quirk; utils/detect_batch.box_iou_darknet's
known answers, darknet_unmap against the repository's own exact inverse, and anchor_detect_classes_darknet /
match_image_f on hand-made candidates.  tests/test_gpu_darknet_protocol.py holds the kernels to these functions."""
import numpy as np
import pytest

from tensorflow_yolo2_amd.img_dataset import pascal_voc as PV
from tensorflow_yolo2_amd.utils import detect_batch as DB

F = np.float32

# (height, width, size): bars on either side, no bar, extents of 1 in both directions, the quirk pair, upscale, downscale
LOOP_CASES = ((5, 7, 32), (7, 5, 32), (12, 9, 32), (3, 20, 32), (1, 9, 32), (9, 1, 32), (6, 25, 32), (8, 21, 64),
              (21, 8, 64), (33, 33, 32), (75, 100, 64), (100, 75, 96), (1, 40, 32))


def _image(h, w, seed=0):
    return np.random.default_rng(1000 * h + w + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def letterbox_darknet_loops(img, size):
    """Darknet's letterbox_image, loop by loop in scalar float32: fill, resize_image's two passes, embed"""
    H, W = img.shape[:2]
    new_w, new_h, ox, oy = PV.letterbox_geometry(H, W, size)
    src = np.empty((H, W, 3), F)
    for y in range(H):
        for x in range(W):
            for k in range(3):
                src[y, x, k] = F(img[y, x, 2 - k]) / F(255.0)
    part = np.zeros((H, new_w, 3), F)
    w_scale = F(W - 1) / F(new_w - 1) if new_w > 1 else F(0.0)
    h_scale = F(H - 1) / F(new_h - 1) if new_h > 1 else F(0.0)
    for k in range(3):
        for r in range(H):
            for c in range(new_w):
                if c == new_w - 1 or W == 1:
                    val = src[r, W - 1, k]
                else:
                    sx = F(c) * w_scale
                    ix = int(sx)
                    dx = F(sx - F(ix))
                    val = F(F(F(1.0) - dx) * src[r, ix, k]) + F(dx * src[r, min(ix + 1, W - 1), k])
                part[r, c, k] = val
    pic = np.zeros((new_h, new_w, 3), F)
    for k in range(3):
        for r in range(new_h):
            sy = F(r) * h_scale
            iy = int(sy)
            dy = F(sy - F(iy))
            for c in range(new_w):
                pic[r, c, k] = F(F(F(1.0) - dy) * part[min(iy, H - 1), c, k])
            if r == new_h - 1 or H == 1:
                continue
            for c in range(new_w):
                pic[r, c, k] = F(pic[r, c, k] + F(dy * part[min(iy + 1, H - 1), c, k]))
    out = np.full((size, size, 3), 0.5, F)
    for y in range(new_h):
        for x in range(new_w):
            for k in range(3):
                out[oy + y, ox + x, k] = pic[y, x, k]
    return out


@pytest.mark.parametrize("h,w,size", LOOP_CASES)
def test_letterbox_darknet_is_the_loop_by_loop_restatement(h, w, size):
    img = _image(h, w)
    got = PV.letterbox_darknet(img, size)
    want = letterbox_darknet_loops(img, size)
    assert got.dtype == np.float32 and got.shape == (size, size, 3)
    assert np.isfinite(got).all()                                         # extents of 1 included
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the bars are exactly 0.5 and the picture is exactly the rectangle the geometry names
    new_w, new_h, ox, oy = PV.letterbox_geometry(h, w, size)
    mask = np.zeros((size, size), bool)
    mask[oy:oy + new_h, ox:ox + new_w] = True
    assert (got[~mask] == F(0.5)).all()
    black = PV.letterbox_darknet(np.zeros_like(img), size)                # a picture that is nowhere 0.5
    assert np.array_equal(black[..., 0] == 0, mask)


def test_resizing_to_the_images_own_size_returns_the_source():
    for n in (32, 64):
        img = _image(n, n, 3)
        src = img[:, :, ::-1].astype(F) / F(255.0)
        assert np.array_equal(PV.letterbox_darknet(img, n).view(np.uint32), src.view(np.uint32))


def test_last_column_is_the_sources_last_column_where_rows_map_to_rows():
    # 16 x 50 at 32: new_w = 32, new_h = 10; horizontal pass alone decides the last column of `part`; rows 0 of the picture
    # is row 0 of the source (sy = 0, dy = 0), so the picture's top right pixel is the source's
    for (h, w, size) in ((16, 50, 32), (9, 40, 64), (33, 33, 32)):
        img = _image(h, w, 5)
        new_w, new_h, ox, oy = PV.letterbox_geometry(h, w, size)
        got = PV.letterbox_darknet(img, size)
        src = img[:, :, ::-1].astype(F) / F(255.0)
        assert np.array_equal(got[oy, ox + new_w - 1], src[0, w - 1])
    # and with the height kept (h = new_h) the whole column
    img = _image(32, 20, 6)
    got = PV.letterbox_darknet(img, 32)
    new_w, new_h, ox, oy = PV.letterbox_geometry(32, 20, 32)
    assert new_h == 32 and np.array_equal(got[:, ox + new_w - 1], (img[:, :, ::-1].astype(F) / F(255.0))[:, 19])


def test_the_last_row_quirk_is_restated_not_repaired():
    """(im_h, new_h) = (8, 24): float(23) * (float(7) / float(23)) rounds below 7, so the last row is (1 - dy) * part(6)
    with dy ~ 1, and never receives the second term: nearly black.  20 x 8 gives new_h = 25, which has no such rounding"""
    assert F(23) * (F(7) / F(23)) < F(7)
    white = np.full((8, 21, 3), 255, np.uint8)
    assert PV.letterbox_geometry(8, 21, 64) == (64, 24, 0, 20)
    got = PV.letterbox_darknet(white, 64)
    assert (got[20:43] == 1).all() and (got[43] < 1e-6).all() and (got[44:] == F(0.5)).all()
    white = np.full((8, 20, 3), 255, np.uint8)
    assert PV.letterbox_geometry(8, 20, 64) == (64, 25, 0, 19)
    got = PV.letterbox_darknet(white, 64)
    assert (got[19:44] == 1).all()


def test_extents_of_one_are_finite_and_copied():
    row = _image(1, 40, 1)                                                # new_h = 1 at 32: the scale is taken as 0
    got = PV.letterbox_darknet(row, 32)
    assert PV.letterbox_geometry(1, 40, 32) == (32, 1, 0, 15) and np.isfinite(got).all()
    col = _image(40, 1, 2)
    got = PV.letterbox_darknet(col, 32)
    assert PV.letterbox_geometry(40, 1, 32) == (1, 32, 15, 0) and np.isfinite(got).all()
    src = col[:, :, ::-1].astype(F) / F(255.0)
    assert np.array_equal(got[0, 15], src[0, 0])


# ---- boxes
def test_box_iou_darknet_known_answers():
    a = np.array([10, 10, 4, 4], F)
    b = np.array([[10, 10, 4, 4],      # identical
                  [20, 20, 4, 4],      # disjoint
                  [10, 10, 2, 2],      # nested
                  [14, 10, 4, 4],      # touching: overlap 0 in x
                  [11, 10, 4, 4]], F)  # half a box apart: 12 / 20
    got = DB.box_iou_darknet(a, b)
    assert got.dtype == np.float32
    assert got.tolist() == [1.0, 0.0, 0.25, 0.0, F(12) / F(20)]
    z = np.array([5, 5, 0, 0], F)                                         # zero area against itself: 0 / 0
    nan = DB.box_iou_darknet(z, z[None])
    assert np.isnan(nan).all() and not (nan > F(0.0)).any()               # a NaN suppresses nothing
    assert DB.box_iou_darknet(a, np.zeros((0, 4), F)).shape == (0,)


@pytest.mark.parametrize("im_h,im_w", ((333, 500), (500, 375), (240, 352), (97, 150), (416, 416)))
@pytest.mark.parametrize("size", (416, 608, 64))
def test_darknet_unmap_against_the_repositorys_exact_inverse(im_h, im_w, size):
    rng = np.random.default_rng(im_h + size)
    boxes = np.concatenate([rng.uniform(0.0, 1.0, (200, 2)), rng.uniform(0.01, 0.9, (200, 2))], axis=1).astype(F)
    got = DB.darknet_unmap(boxes, im_w, im_h, size)
    assert got.dtype == np.float32 and got.shape == (200, 4)
    ours = DB._letterbox_products(boxes, im_w, im_h, size)
    new_w, new_h, ox, oy = PV.letterbox_geometry(im_h, im_w, size)
    # Darknet's half offset (N - new) / 2. is up to half a canvas pixel from the integer bar the picture was embedded
    # at: half a canvas pixel is 0.5 * im / new pixels of the image; 1e-3 covers the float32 roundings at these sizes
    d = np.abs(got.astype(np.float64) - ours)
    assert (d[:, 0] <= 0.5 * im_w / new_w + 1e-3).all() and (d[:, 1] <= 0.5 * im_h / new_h + 1e-3).all()
    assert (d[:, 2] <= 1e-3).all() and (d[:, 3] <= 1e-3).all()
    # where the bar is whole pixels the two maps are one, up to float32 rounding: a few ulp of a value below 2 * im
    tol_x = 16 * np.spacing(F(2 * im_w))
    tol_y = 16 * np.spacing(F(2 * im_h))
    if (size - new_w) % 2 == 0:
        assert (d[:, 0] <= tol_x).all(), d[:, 0].max()
    if (size - new_h) % 2 == 0:
        assert (d[:, 1] <= tol_y).all(), d[:, 1].max()
    with pytest.raises(ValueError, match="net_size"):
        DB.darknet_unmap(boxes, im_w, im_h, size + 1)


def _rel(px_box, im_w, im_h, size):
    """a centre box in pixels of the image -> relative to the letterboxed canvas (the inverse of darknet_unmap, double)"""
    new_w, new_h, _, _ = PV.letterbox_geometry(im_h, im_w, size)
    x, y, w, h = px_box
    return [(x / im_w) * (new_w / size) + (size - new_w) / 2.0 / size, (y / im_h) * (new_h / size) + (size - new_h) / 2.0 / size,
            (w / im_w) * (new_w / size), (h / im_h) * (new_h / size)]


def hand_made_image():
    """(boxes [K][4] relative, scores [K][3], im_w, im_h, size, names): class 0 holds a kept box, one it suppresses, a tie
    of two boxes apart, a NaN score and a box that lies in the top bar; class 1 four boxes apart for a cap of 3; class 2
    a box with an infinite width"""
    im_w, im_h, size = 200, 100, 64                                       # new_h = 32: bars of 16 rows
    px = [(50, 50, 40, 40), (52, 50, 40, 40), (150, 30, 20, 20), (150, 70, 20, 20), (100, 50, 10, 10),
          (100, -30, 20, 20),                                             # 5: wholly in the top bar (above the image)
          (20, 20, 10, 10), (60, 20, 10, 10), (100, 20, 10, 10), (140, 20, 10, 10),
          (100, 50, np.inf, 10)]
    boxes = np.array([_rel(b, im_w, im_h, size) for b in px], F)
    scores = np.zeros((len(px), 3), F)
    scores[:6, 0] = (0.9, 0.8, 0.5, 0.5, np.nan, 0.7)
    scores[6:10, 1] = (0.6, 0.7, 0.8, 0.9)
    scores[10, 2] = 0.9
    return boxes, scores, im_w, im_h, size


def test_anchor_detect_classes_darknet_on_a_hand_made_image():
    boxes, scores, im_w, im_h, size = hand_made_image()
    M = 3
    det, score, count = DB.anchor_detect_classes_darknet(boxes, scores, im_w, im_h, 0.1, 0.45, M, size)
    assert det.dtype == np.int32 and det.shape == (3, M, 6) and score.shape == (3, M) and count.tolist() == [3, 3, 0]
    # class 0: 0 kept, 1 suppressed by it, the bar box next (0.7: nothing drops it, it is cut to an EMPTY box and kept),
    # then the tie 2, 3 in candidate order -- the cap of 3 ends the walk after candidate 2
    assert det[0, :, 5].tolist() == [0, 5, 2] and det[0, :, 4].tolist() == [0, 0, 0]
    assert score[0].tolist() == [F(0.9), F(0.7), F(0.5)]
    full = DB.anchor_detect_classes_darknet(boxes, scores, im_w, im_h, 0.1, 0.45, 10, size)
    assert full[2].tolist() == [4, 4, 0] and full[0][0, :4, 5].tolist() == [0, 5, 2, 3]      # tie: ascending candidate
    assert (full[0][0, 4:] == -1).all() and (full[1][0, 4:] == 0).all()
    corners = det[0, :, :4].copy().view(np.float32)
    assert np.allclose(corners[0], [31, 31, 71, 71], atol=1e-3)          # centre 50 -/+ 20, + 1
    assert corners[1, 1] == 1.0 and corners[1, 3] < corners[1, 1]         # the bar box: ymin raised to 1, ymax below it
    # class 1: the cap is reached (saturated), in descending score
    assert det[1, :, 5].tolist() == [9, 8, 7] and count[1] == M
    # class 2: an infinite width is not valid; NaN scores compare false (candidate 4 never appears)
    assert 4 not in full[0][0, :, 5].tolist() and count[2] == 0
    # a NaN IoU suppresses nothing: two zero-area boxes at one point are both kept
    z = np.array([_rel((50, 50, 0, 0), im_w, im_h, size)] * 2, F)
    d, s, c = DB.anchor_detect_classes_darknet(z, np.array([[0.9], [0.8]], F), im_w, im_h, 0.1, 0.0, 5, size)
    assert c.tolist() == [2]


def test_match_image_f_reads_float_corners_and_keeps_match_images_rules():
    gt = np.array([[10, 10, 50, 50, 0], [100, 100, 150, 150, 0], [10, 10, 50, 50, 1]], np.float64)
    difficult = [0, 1, 0]
    rows = np.array([[10.25, 10.5, 50.0, 49.75], [10.0, 10.0, 50.0, 50.0], [100.5, 100.0, 150.0, 150.0],
                     [10.0, 10.0, 50.0, 29.49], [10.0, 10.0, 50.0, 29.51], [10.0, 10.0, 50.0, 50.0]], F)
    cls = np.array([0, 0, 0, 0, 0, 2])
    det = np.full((6, 6), -1, np.int32)
    det[:, :4] = rows.view(np.int32)
    det[:, 4] = cls
    flags = DB.match_image_f(det, gt, difficult, 0.5)
    # true positive; the object is taken; difficult: ignored; IoU just below and just above one half of a taken object
    # (false positives both, but the second one ONLY because the object is taken); a class without objects
    assert flags.tolist() == [1, 0, 2, 0, 0, 0]
    assert DB.match_image_f(det[4:5], gt, difficult, 0.5).tolist() == [1]
    assert DB.match_image_f(det[3:4], gt, difficult, 0.5).tolist() == [0]
    # float rows and bit patterns agree, and integer-valued float rows get match_image's flags
    as_float = np.concatenate([rows, cls[:, None].astype(F)], axis=1)
    assert DB.match_image_f(as_float, gt, difficult, 0.5).tolist() == flags.tolist()
    ints = np.array([[10, 10, 50, 50, 0, 0], [12, 10, 50, 50, 1, 1]], np.int32)
    f = ints.copy()
    f[:, :4] = ints[:, :4].astype(F).view(np.int32)
    assert DB.match_image_f(f, gt, difficult).tolist() == DB.match_image(ints, gt, difficult).tolist() == [1, 1]
    assert DB.match_image_f(np.zeros((0, 6), np.int32), gt, difficult).shape == (0,)


def test_results_files_print_float_rows_with_percent_f(tmp_path):
    from tensorflow_yolo2_amd.utils import voc_eval
    rows = {"image": [0, 1], "class": [0, 0], "score": np.array([0.5, 0.25], F),
            "box": np.array([[1.0, 2.5, 30.125, 40.0], [3.0, 4.0, 5.0, 6.0]], F)}
    paths = voc_eval.write_results_files(str(tmp_path / "f"), "test", ["a", "b"], ["aeroplane"], rows)
    assert open(paths[0]).read() == ("a 0.500000 1.000000 2.500000 30.125000 40.000000\n"
                                     "b 0.250000 3.000000 4.000000 5.000000 6.000000\n")
    rows["box"] = np.array([[1, 2, 30, 40], [3, 4, 5, 6]], np.int32)      # integer rows print exactly as before
    paths = voc_eval.write_results_files(str(tmp_path / "i"), "test", ["a", "b"], ["aeroplane"], rows)
    assert open(paths[0]).read() == "a 0.500000 1 2 30 40\nb 0.250000 3 4 5 6\n"


def test_protocol_darknet_argument_errors_of_the_two_scripts():
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2, pascal_eval_yolov2
    ev = ["--devkit", "kit"]
    a = pascal_eval_yolov2.parse_args(ev + ["--darknet-weights", "f.weights", "--protocol", "darknet"])
    assert a.per_class and a.letterbox and a.fill == 127 and a.protocol == "darknet"      # it implies the two switches
    d = pascal_eval_yolov2.parse_args(ev)
    assert d.protocol == "repo" and d.fill == 127 and not d.per_class and not d.letterbox  # the defaults are today's
    assert pascal_eval_yolov2.parse_args(ev + ["--letterbox", "--fill", "3"]).fill == 3
    for bad in (["--darknet-weights", "f.weights", "--protocol", "darknet", "--fill", "127"],
                ["--weights", "x.npz", "--protocol", "darknet"], ["--protocol", "darknet"], ["--protocol", "other"]):
        with pytest.raises(SystemExit):
            pascal_eval_yolov2.parse_args(ev + bad)
    im = ["--images", "a.jpg"]
    assert pascal_detect_yolov2.parse_args(im + ["--darknet-weights", "f.weights", "--protocol", "darknet"]).fill == 127
    assert pascal_detect_yolov2.parse_args(im).protocol == "repo"
    for bad in (["--darknet-weights", "f.weights", "--protocol", "darknet", "--stretch"],
                ["--darknet-weights", "f.weights", "--protocol", "darknet", "--fill", "0"], ["--protocol", "darknet"]):
        with pytest.raises(SystemExit):
            pascal_detect_yolov2.parse_args(im + bad)


def test_quotient_by_255_from_one_product_and_one_correction_is_the_division():
    """the kernel forms float(b) / 255 as q0 = b * r, q = fma(fma(-255, q0, b), r, q0) with r = float32(1 / 255): in exact
    rational arithmetic, rounded to float32 where the hardware rounds, that is the correctly rounded quotient for every
    byte -- the value letterbox_darknet divides out"""
    from fractions import Fraction as Fr

    def rnd(x):                                                           # Fraction -> nearest float32
        d = float(x)                                                      # correctly rounded to float64 first
        s = F(d)
        if Fr(d) != x:                                                    # then no float32 tie may hide in that rounding
            for o in (np.nextafter(s, F(-np.inf)), np.nextafter(s, F(np.inf))):
                assert Fr(d) != (Fr(float(s)) + Fr(float(o))) / 2
        return s
    r = F(1.0) / F(255.0)
    assert r.view(np.uint32) == 0x3b808081
    for b in range(256):
        q0 = rnd(Fr(b) * Fr(float(r)))
        rem = rnd(Fr(b) - 255 * Fr(float(q0)))
        assert Fr(float(rem)) == Fr(b) - 255 * Fr(float(q0))              # the remainder is exact
        q = rnd(Fr(float(rem)) * Fr(float(r)) + Fr(float(q0)))
        assert q == F(b) / F(255.0), b
