"""Letterboxed inference of the YOLOv2 anchor detector, host side (no GPU): the one geometry (pascal_voc.letterbox_geometry,
the restatement of csrc/letterbox.h), the image specification pascal_voc.letterbox_u8 (of y2_letterbox_u8_batch) and the
inverse map of utils/detect_batch.anchor_candidates(net_size=N) (of y2_detect_anchor_batch_lb and
y2_detect_anchor_classes_batch_lb).  Everything but the round trip is equality; the round trip's bound of one pixel is
the truncation toward zero of the decode (the float32 relative box moves a product by less than 1e-4 pixels)."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_detect_anchor import ANCHORS, SHAPES, _anchor_case
from tensorflow_yolo2_amd.img_dataset import pascal_voc as PV
from tensorflow_yolo2_amd.utils import detect_batch as DB

#            width, height, size -> new_w, new_h, ox, oy
GEOMETRY = ((500, 375, 416, (416, 312, 0, 52)),
            (375, 500, 416, (312, 416, 52, 0)),
            (150, 97, 64, (64, 41, 0, 11)),            # 64 - 41 = 23: bars of 11 and 12, the odd pixel at the bottom
            (97, 150, 64, (41, 64, 11, 0)),
            (64, 64, 96, (96, 96, 0, 0)),              # square: no bars
            (500, 1, 416, (416, 1, 0, 207)),           # 1 * 416 / 500 = 0: clamped to one row
            (1, 200, 32, (1, 32, 15, 0)),
            (2147483647, 2147483647, 608, (608, 608, 0, 0)),
            (2147483647, 3, 608, (608, 1, 0, 303)))    # products beyond 2^32


@pytest.mark.parametrize("im_w,im_h,size,want", GEOMETRY)
def test_geometry(im_w, im_h, size, want):
    assert PV.letterbox_geometry(im_h, im_w, size) == want
    new_w, new_h, ox, oy = want
    assert max(new_w, new_h) == size and 0 <= size - new_w - 2 * ox <= 1 and 0 <= size - new_h - 2 * oy <= 1


def test_library_geometry_is_the_python_one():
    """y2_letterbox_geometry is host-only: the header function the kernels call, without a GPU"""
    from tensorflow_yolo2_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libyolo2_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    out = (C.c_int * 4)()
    rng = np.random.default_rng(5)
    cases = [(h, w, n) for (w, h, n, _g) in GEOMETRY]
    cases += [tuple(int(v) for v in rng.integers(1, 700, 2)) + (int(32 * rng.integers(1, 20)),) for _ in range(200)]
    for im_h, im_w, size in cases:
        assert lib.y2_letterbox_geometry(im_h, im_w, size, out) == 0
        assert tuple(out) == PV.letterbox_geometry(im_h, im_w, size), (im_h, im_w, size)
    for bad in ((0, 5, 32), (5, 0, 32), (5, 5, 0), (-1, 5, 32)):
        assert lib.y2_letterbox_geometry(*bad, out) == -1 and b"y2_letterbox_geometry" in lib.y2_last_error()
    assert lib.y2_letterbox_geometry(5, 5, 32, None) == -1 and b"null" in lib.y2_last_error()


def test_letterbox_u8_is_the_resize_inside_and_the_fill_outside():
    rng = np.random.default_rng(11)
    square = rng.integers(0, 256, (50, 50, 3), dtype=np.uint8)
    for size in (32, 64, 96):
        assert np.array_equal(PV.letterbox_u8(square, size), PV.resize_bilinear_u8(square, size, size))
    for (h, w), size, fill in (((97, 150), 64, 127), ((150, 97), 64, 0), ((1, 200), 32, 255), ((333, 500), 96, 3)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[0], img[-1], img[:, 0], img[:, -1] = 255 - fill, 255 - fill, 255 - fill, 255 - fill   # an edge far from the fill
        new_w, new_h, ox, oy = PV.letterbox_geometry(h, w, size)
        out = PV.letterbox_u8(img, size, fill)
        assert out.shape == (size, size, 3) and out.dtype == np.uint8
        inside = np.zeros((size, size), bool)
        inside[oy:oy + new_h, ox:ox + new_w] = True
        assert (~inside).any() and (out[~inside] == fill).all()
        # the rectangle is the resize of the image alone: no fill bleeds into it
        assert np.array_equal(out[oy:oy + new_h, ox:ox + new_w], PV.resize_bilinear_u8(img, new_h, new_w))
    assert PV.letterbox_u8(square, 32).min() >= 0 and PV.letterbox_u8(square[:10], 32)[0, 0].tolist() == [127] * 3


def test_net_size_none_is_the_call_without_the_keyword():
    from oracle import ext_ref as X
    S, B, ncls = 7, 3, 1
    net, _named = _anchor_case(S, B, ncls)
    boxes, scores = X.decode_anchors(net, ANCHORS[:B])
    with np.errstate(all="ignore"):
        best, cls = scores.max(axis=2), scores.argmax(axis=2)
    for img, (h, w) in enumerate(SHAPES[:3]):
        for a, b in zip(DB.anchor_candidates(boxes[img], best[img], cls[img], w, h, 0.2),
                        DB.anchor_candidates(boxes[img], best[img], cls[img], w, h, 0.2, net_size=None)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        for a, b in zip(DB.anchor_detect(boxes[img], best[img], cls[img], w, h, 0.2, 0.45, 24),
                        DB.anchor_detect(boxes[img], best[img], cls[img], w, h, 0.2, 0.45, 24, net_size=None)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
        for a, b in zip(DB.anchor_detect_classes(boxes[img], scores[img], w, h, 0.02, 0.45, 8),
                        DB.anchor_detect_classes(boxes[img], scores[img], w, h, 0.02, 0.45, 8, net_size=None)):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    # and the letterbox map is another map: on a non-square image the rows differ
    h, w = SHAPES[0]
    assert not np.array_equal(DB.anchor_candidates(boxes[0], best[0], cls[0], w, h, 0.2)[1],
                              DB.anchor_candidates(boxes[0], best[0], cls[0], w, h, 0.2, net_size=32 * S)[1])


def _forward(box, im_w, im_h, size):
    """the 1-based inclusive source box -> (cx, cy, w, h) relative to the letterboxed canvas, in float64: the embedding
    takes source pixel x to canvas x / sx + ox; the centre is the one anchor_candidates' corner rule inverts"""
    new_w, new_h, ox, oy = PV.letterbox_geometry(im_h, im_w, size)
    sx, sy = im_w / new_w, im_h / new_h
    x0, y0, x1, y1 = box
    bw, bh = x1 - x0 + 1, y1 - y0 + 1
    cx, cy = x0 - 1 + bw // 2 + 0.5, y0 - 1 + bh // 2 + 0.5
    return ((cx / sx + ox) / size, (cy / sy + oy) / size, (bw + 0.5) / sx / size, (bh + 0.5) / sy / size)


@pytest.mark.parametrize("size", (64, 416, 608))
@pytest.mark.parametrize("shape", SHAPES)
def test_round_trip_through_the_inverse_map(shape, size):
    im_h, im_w = shape
    rng = np.random.default_rng(im_h * 1000 + size)
    boxes = [(1, 1, im_w, im_h), (1, 1, 1, 1), (im_w, im_h, im_w, im_h), (1, 1, 2, 3), (im_w - 10, 5, im_w, 40)]
    for _ in range(60):
        x0, y0 = int(rng.integers(1, im_w + 1)), int(rng.integers(1, im_h + 1))
        boxes.append((x0, y0, int(rng.integers(x0, im_w + 1)), int(rng.integers(y0, im_h + 1))))
    rel = np.array([_forward(b, im_w, im_h, size) for b in boxes])
    valid, got, _cls, _score = DB.anchor_candidates(rel, np.ones(len(boxes), np.float32), np.zeros(len(boxes)), im_w,
                                                    im_h, 0.5, net_size=size)
    assert valid.all()
    diff = np.abs(got - np.array(boxes))
    print("round trip %d x %d at %d: largest edge difference %d pixel(s)" % (im_w, im_h, size, diff.max()))
    assert diff.max() <= 1
    assert (got[:, 0] >= 1).all() and (got[:, 1] >= 1).all() and (got[:, 2] <= im_w).all() and (got[:, 3] <= im_h).all()


def test_a_box_in_a_bar_is_dropped_and_one_across_its_edge_is_cut():
    im_w, im_h, size = 500, 375, 416                                      # rows 0..51 and 364..415 of the canvas are bars
    new_w, new_h, ox, oy = PV.letterbox_geometry(im_h, im_w, size)
    assert (new_w, new_h, ox, oy) == (416, 312, 0, 52)
    rel = np.array([(210.0, 20.0, 60.0, 30.0),                            # rows 5 .. 35: wholly in the top bar
                    (210.0, 390.0, 60.0, 30.0),                           # wholly in the bottom bar
                    (210.0, 52.0, 60.0, 40.0),                            # rows 32 .. 72: across the top bar's edge
                    (210.0, 364.0, 60.0, 40.0),                           # across the bottom bar's edge
                    (210.0, 208.0, 60.0, 40.0)]) / size                   # inside the picture
    valid, box, _cls, _score = DB.anchor_candidates(rel, np.ones(5, np.float32), np.zeros(5), im_w, im_h, 0.5,
                                                    net_size=size)
    assert valid.tolist() == [False, False, True, True, True]
    assert (box[:2] == 0).all()
    sy = im_h / new_h
    assert box[2].tolist() == [217, 1, 288, int(20 * sy)] and box[3, 3] == im_h and box[3, 1] > im_h - 30
    assert box[4].tolist() == [217, 164, 288, 211]
    # the plain stretch keeps all five: the bars are its picture
    assert DB.anchor_candidates(rel, np.ones(5, np.float32), np.zeros(5), im_w, im_h, 0.5)[0].all()
    # the same through both walks
    det, _s = DB.anchor_detect(rel, np.ones(5, np.float32), np.zeros(5), im_w, im_h, 0.5, 0.45, 10, net_size=size)
    assert sorted(det[:, 5].tolist()) == [2, 3, 4]
    _d, _s, count = DB.anchor_detect_classes(rel, np.ones((5, 2), np.float32), im_w, im_h, 0.5, 0.45, 10, net_size=size)
    assert count.tolist() == [3, 3]


@pytest.mark.parametrize("net_size", (0, -32, 100, 33, 416.5))
def test_net_size_must_be_a_positive_multiple_of_32(net_size):
    with pytest.raises(ValueError, match="net_size"):
        DB.anchor_candidates(np.zeros((1, 4)), np.ones(1), np.zeros(1), 10, 10, 0.5, net_size=net_size)


def test_geometry_and_fill_refusals():
    for bad in ((0, 10, 32), (10, 0, 32), (10, 10, 0)):
        with pytest.raises(ValueError, match="letterbox_geometry"):
            PV.letterbox_geometry(*bad)
    for fill in (-1, 256):
        with pytest.raises(ValueError, match="fill"):
            PV.letterbox_u8(np.zeros((4, 4, 3), np.uint8), 32, fill)


def test_device_images_layout_with_the_upload_stubbed(golden_dir, monkeypatch):
    """the pool and the entry table of DeviceVOC, from files alone"""
    from tensorflow_yolo2_amd.img_dataset import device_images as DI
    pools, uploads = [], []
    monkeypatch.setattr(DI.DeviceImages, "_alloc_pool", lambda self, n: pools.append(np.zeros(n, np.uint8)) or pools[-1])
    monkeypatch.setattr(DI.DeviceImages, "_put", lambda self, pool, off, flat: pool.__setitem__(slice(off, off + flat.size), flat))
    monkeypatch.setattr(DI.DeviceImages, "_upload", lambda self, a: uploads.append(np.array(a)) or uploads[-1])
    paths = [os.path.join(golden_dir, n) for n in ("testImg2.jpg", "testImg1.jpg")]
    ds = DI.DeviceImages(paths, 2, device="cpu")
    table = uploads[0]
    assert table.dtype == np.int64 and table.tolist() == [[0, 500, 353, 1072, 0], [500 * 1072, 240, 352, 1056, 0]]
    assert ds.pool_bytes == pools[0].size == 500 * 1072 + 240 * 1056
    for k, p in enumerate(paths):
        off, h, w, pitch = table[k, :4]
        rows = pools[0][off:off + h * pitch].reshape(h, pitch)
        assert np.array_equal(rows[:, :3 * w].reshape(h, w, 3), PV.imread_bgr(p)) and not rows[:, 3 * w:].any()
    with pytest.raises(RuntimeError, match="DeviceImages.batch needs the pool on the GPU"):
        ds.batch(64, 0)
    with pytest.raises(ValueError, match="at least one"):
        DI.DeviceImages([], 2)
    with pytest.raises(MemoryError):
        DI.DeviceImages(paths, 2, device="cpu", max_pool_bytes=1000)


def test_detect_script_refuses_sizes_the_head_cannot_take():
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2 as D
    for argv in (["--images", "a.jpg", "--size", "100"], ["--images", "a.jpg", "--size", "672"],
                 ["--images", "a.jpg", "--fill", "256"], ["--size", "416"]):
        with pytest.raises(SystemExit):
            D.parse_args(argv)
    args = D.parse_args(["--images", "a.jpg", "b.jpg"])
    assert (args.size, args.thresh, args.nms, args.stretch, args.batch, args.fill) == (416, 0.24, 0.45, False, 2, 127)
