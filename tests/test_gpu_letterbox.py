"""Letterboxed inference of the YOLOv2 anchor detector on the device: y2_letterbox_u8_batch (csrc/data.hip) bit for bit
against pascal_voc.letterbox_u8, y2_detect_anchor_batch_lb and y2_detect_anchor_classes_batch_lb (csrc/detect.hip) bit
for bit against utils/detect_batch.anchor_detect / anchor_detect_classes with net_size, fed with the device's own
y2_decode_anchors, and pascal_eval_yolov2 --letterbox and pascal_detect_yolov2 against the host composition on the same
head outputs.  Everything is equality: no tolerance.  tests/test_letterbox_host.py holds what needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from test_device_voc_host import make_devkit
from test_gpu_detect_anchor import (ANCHORS, IOU_THRESH, MAX_OUT, SCORE_THRESH, SHAPES, _anchor_case, _host_rows, _table,
                                    _unit_gain_layers)
from test_gpu_detect_anchor_classes import MAX_PER_CLASS, MIXED_THRESH
from tensorflow_yolo2_amd.img_dataset import pascal_voc as PV
from tensorflow_yolo2_amd.utils import detect_batch as DB

gpu = pytest.mark.gpu

# (height, width) of the hand-made pool's entries: a bar narrower than a band of 16 output rows (97 x 150 at 64: 11 and
# 12), bars left and right, no bar, new_h clamped to 1, an image wider than every output, a bar of ONE pixel (150 x 160
# at 32: rows 1 .. 30), and a row of more than 4096 bytes, which the kernel reads in place instead of staging it
POOL_SHAPES = ((97, 150), (150, 97), (64, 64), (1, 200), (333, 500), (150, 160), (30, 1400))
REORDER = (4, 0, 6, 6, 3, 1, 5, 2, 0)
LB_GEOMETRIES = ((1, 5, 20), (7, 3, 1), (19, 5, 20))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def pool():
    """(images, pool uint8 device tensor, table int64 device tensor): random bytes, DeviceVOC's layout"""
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_voc import padded_rows, pool_layout
    rng = np.random.default_rng(77)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in POOL_SHAPES]
    offsets, pitches, total = pool_layout(POOL_SHAPES)
    assert pitches[-1] > 4096 and max(pitches[:-1]) <= 4096
    flat = np.zeros(total, np.uint8)
    for img, off, pitch in zip(images, offsets, pitches):
        flat[off:off + img.shape[0] * pitch] = padded_rows(img, pitch).reshape(-1)
    table = np.array([(off, h, w, pitch, 0) for (h, w), off, pitch in zip(POOL_SHAPES, offsets, pitches)], np.int64)
    return images, torch.from_numpy(flat).cuda(), torch.from_numpy(table).cuda()


@gpu
@pytest.mark.parametrize("size", (32, 64, 96))
def test_letterbox_batch_is_bit_equal_to_the_specification(pool, size):
    import torch
    from tensorflow_yolo2_amd import engine as E
    images, dev_pool, table = pool
    geo = [PV.letterbox_geometry(h, w, size) for (h, w) in POOL_SHAPES]
    if size == 64:
        assert geo[0] == (64, 41, 0, 11) and geo[1] == (41, 64, 11, 0)
    if size == 32:
        assert geo[3] == (32, 1, 0, 15) and geo[5] == (32, 30, 0, 1)
    assert geo[2] == (size, size, 0, 0)
    for fill in (0, 127, 255):
        want = [PV.letterbox_u8(img, size, fill) for img in images]
        for index in (None, REORDER):
            entries = list(index) if index is not None else list(range(len(images)))
            idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
            for sentinel in (0x5A, 0xA5):                                 # every byte is written, whatever it held
                out = torch.full((len(entries), size, size, 3), sentinel, dtype=torch.uint8, device="cuda")
                got = E.letterbox_batch(dev_pool, table, idx, len(entries), size, fill, out=out)
                torch.cuda.synchronize()
                assert got is out
                got = got.cpu().numpy()
                for k, e in enumerate(entries):
                    assert np.array_equal(got[k], want[e]), (size, fill, index is not None, k, e)


@gpu
def test_letterbox_batch_argument_errors():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    #           n  size  fill
    for case, word in (((0, 64, 127), b"n = 0"), ((65536, 64, 127), b"n = 65536"), ((1, 0, 127), b"size = 0"),
                       ((1, 66, 127), b"size = 66"), ((1, 1028, 127), b"size = 1028"), ((1, 64, -1), b"fill = -1"),
                       ((1, 64, 256), b"fill = 256")):
        n, size, fill = case
        assert lib.y2_letterbox_u8_batch(p, p, None, n, size, fill, p, None) == -1, case
        assert b"y2_letterbox_u8_batch" in lib.y2_last_error() and word in lib.y2_last_error(), lib.y2_last_error()
    for null in (0, 1, 6):
        a = [p, p, None, 1, 64, 127, p, None]
        a[null] = None
        assert lib.y2_letterbox_u8_batch(*a) == -1 and b"null" in lib.y2_last_error()
    assert lib.y2_letterbox_u8_batch(p, p, None, 1, 64, 127, C.c_void_p(buf.data_ptr() + 2), None) == -1
    assert b"aligned" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


def _new_ground(boxes, score, im_w, im_h, size, thresh):
    """(dropped, cut): candidates whose score passes and whose box, of 2 to `size` pixels and inside the canvas, lies
    (by more than a pixel) wholly in a bar and is not valid / reaches (by more than a pixel) across the picture's edge
    into a bar and is valid: what the letterbox map adds to the rules"""
    new_w, new_h, ox, oy = PV.letterbox_geometry(im_h, im_w, size)
    valid = DB.anchor_candidates(boxes, score, np.zeros(len(boxes)), im_w, im_h, thresh, net_size=size)[0]
    with np.errstate(all="ignore"):
        b = boxes.astype(np.float64) * size
        passes = (score > np.float32(thresh)) & np.isfinite(b).all(axis=1) & (b[:, 2:] >= 2).all(axis=1) & (b[:, 2:] < size).all(axis=1)
        x0, x1, y0, y1 = b[:, 0] - b[:, 2] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 1] + b[:, 3] / 2
        passes &= (x0 >= 0) & (y0 >= 0) & (x1 <= size) & (y1 <= size)
        in_bar = (x1 < ox - 1) | (x0 > ox + new_w + 1) | (y1 < oy - 1) | (y0 > oy + new_h + 1)
        across = (((x0 < ox - 1) & (x1 > ox + 1)) | ((x0 < ox + new_w - 1) & (x1 > ox + new_w + 1)) |
                  ((y0 < oy - 1) & (y1 > oy + 1)) | ((y0 < oy + new_h - 1) & (y1 > oy + new_h + 1)))
    return int((passes & in_bar & ~valid).sum()), int((passes & across & ~in_bar & valid).sum())


def _assert_new_ground(S, B, boxes, best, cls):
    """on the host, before the letterboxed launches: image 0 at entry 0 drops candidates that map into a bar, cuts
    candidates at a bar's edge, and keeps and suppresses rows.  S = 1 is the single-cell launch (a 32-pixel canvas, five
    boxes of anchor size): one box reaches across the edge in image 2, and nothing can lie in a bar of five pixels"""
    size = 32 * S
    if S == 1:
        assert _new_ground(boxes[2], best[2], SHAPES[2][1], SHAPES[2][0], size, SCORE_THRESH)[1] >= 1
        return
    h, w = SHAPES[0]
    dropped, cut = _new_ground(boxes[0], best[0], w, h, size, SCORE_THRESH)
    assert dropped >= 1 and cut >= 1, (dropped, cut)
    valid = DB.anchor_candidates(boxes[0], best[0], cls[0], w, h, SCORE_THRESH, net_size=size)[0]
    kept = len(DB.anchor_detect(boxes[0], best[0], cls[0], w, h, SCORE_THRESH, IOU_THRESH, S * S * B, net_size=size)[0])
    assert 0 < kept < valid.sum()


def _check_anchor_lb(dev, decoded, B, entries, index, score_thresh, iou_thresh, max_out):
    import torch
    from tensorflow_yolo2_amd import engine as E
    size = 32 * dev.shape[1]
    boxes, best, cls = decoded
    table = torch.from_numpy(_table()).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
    n = len(entries)
    out = (torch.full((n, max_out, 6), 77, dtype=torch.int32, device="cuda"),
           torch.full((n, max_out), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    det, score, count = E.detect_anchor_batch(dev, ANCHORS[:B], table, idx, score_thresh, iou_thresh, max_out, out=out,
                                              net_size=size)
    torch.cuda.synchronize()
    det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    for k, e in enumerate(entries):
        want_det, want_score = DB.anchor_detect(boxes[k], best[k], cls[k], SHAPES[e][1], SHAPES[e][0], score_thresh,
                                                iou_thresh, max_out, net_size=size)
        c = len(want_det)
        assert count[k] == c, (k, count[k], c)
        assert np.array_equal(det[k, :c], want_det), k
        assert np.array_equal(score[k, :c].view(np.uint32), want_score.view(np.uint32)), k
        assert (det[k, c:] == -1).all() and (score[k, c:] == 0).all()
    return count


@gpu
@pytest.mark.parametrize("S,B,C", LB_GEOMETRIES)
def test_detect_anchor_lb_is_bit_equal_to_the_specification(S, B, C):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    dev = torch.from_numpy(net).cuda()
    boxes, scores = E.decode_anchors(dev, ANCHORS[:B])
    best, cls = E.class_argmax(scores)
    decoded = tuple(t.cpu().numpy() for t in (boxes, best, cls))
    _assert_new_ground(S, B, *decoded)
    # the sweep of the stretch test (test_gpu_detect_anchor.py)
    _check_anchor_lb(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, IOU_THRESH, MAX_OUT)
    _check_anchor_lb(dev, decoded, B, (3, 1, 1), (3, 1, 1), SCORE_THRESH, IOU_THRESH, MAX_OUT)  # an index, other sizes
    _check_anchor_lb(dev, decoded, B, (2, 0, 3), (2, 0, 3), SCORE_THRESH, IOU_THRESH, K)        # max_out cuts nothing off
    _check_anchor_lb(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, 1.0, K)                    # nothing suppressed
    _check_anchor_lb(dev, decoded, B, (0, 1, 2), (0, 1, 2), -1.0, 0.0, K)        # every score passes, every overlap goes


def _check_classes_lb(dev, decoded, B, entries, index, score_thresh, max_per_class):
    import torch
    from tensorflow_yolo2_amd import engine as E
    size = 32 * dev.shape[1]
    boxes, scores = decoded
    n, ncls = dev.shape[0], dev.shape[4] - 5
    table = torch.from_numpy(_table()).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
    out = (torch.full((n, ncls, max_per_class, 6), 77, dtype=torch.int32, device="cuda"),
           torch.full((n, ncls, max_per_class), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((n, ncls), 77, dtype=torch.int32, device="cuda"))
    got = E.detect_anchor_classes_batch(dev, ANCHORS[:B], table, idx, score_thresh, IOU_THRESH, max_per_class, out=out,
                                        net_size=size)
    torch.cuda.synchronize()
    det, score, count = (t.cpu().numpy() for t in got)
    for k, e in enumerate(entries):
        want = DB.anchor_detect_classes(boxes[k], scores[k], SHAPES[e][1], SHAPES[e][0], score_thresh, IOU_THRESH,
                                        max_per_class, net_size=size)
        assert np.array_equal(count[k], want[2]), (k, count[k], want[2])
        assert np.array_equal(det[k], want[0]), k                         # unused rows are -1 in both
        assert np.array_equal(score[k].view(np.uint32), want[1].view(np.uint32)), k
    return count


@gpu
@pytest.mark.parametrize("S,B,C", LB_GEOMETRIES)
def test_detect_anchor_classes_lb_is_bit_equal_to_the_specification(S, B, C):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    dev = torch.from_numpy(net).cuda()
    boxes, scores = E.decode_anchors(dev, ANCHORS[:B])
    best, cls = E.class_argmax(scores)
    _assert_new_ground(S, B, *(t.cpu().numpy() for t in (boxes, best, cls)))
    decoded = (boxes.cpu().numpy(), scores.cpu().numpy())
    # the sweep of the stretch test (test_gpu_detect_anchor_classes.py)
    for thresh in (0.02, 0.005):
        _check_classes_lb(dev, decoded, B, (0, 1, 2), None, thresh, MAX_PER_CLASS)
        _check_classes_lb(dev, decoded, B, (2, 0, 3), (2, 0, 3), thresh, K)   # an index, other sizes, nothing capped
    _check_classes_lb(dev, decoded, B, (0, 1, 2), None, MIXED_THRESH, MAX_PER_CLASS)
    _check_classes_lb(dev, decoded, B, (0, 1, 2), (0, 1, 2), MIXED_THRESH, K)


@gpu
def test_net_size_that_is_not_32_S_is_an_argument_error():
    import torch
    from tensorflow_yolo2_amd import _lib as L, engine as E
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    for net_size in (0, -416, 415, 448, 384, 32):                        # S = 13: only 416 will do
        assert lib.y2_detect_anchor_batch_lb(p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, net_size, p, p, p, None) == -1
        assert b"y2_detect_anchor_batch_lb: net_size = %d" % net_size in lib.y2_last_error()
        assert lib.y2_detect_anchor_classes_batch_lb(p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, net_size, p, p, p,
                                                     None) == -1
        assert b"y2_detect_anchor_classes_batch_lb: net_size = %d" % net_size in lib.y2_last_error()
    # the other refusals are those of the stretch entries, under the new names
    assert lib.y2_detect_anchor_batch_lb(p, p, p, None, 1, 21, 5, 20, 0.1, 0.5, 10, 672, p, p, p, None) == -1
    assert b"y2_detect_anchor_batch_lb: S * S * B = 2205" in lib.y2_last_error()
    assert lib.y2_detect_anchor_classes_batch_lb(p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 0, 416, p, p, p, None) == -1
    assert b"y2_detect_anchor_classes_batch_lb: max_per_class = 0" in lib.y2_last_error()
    assert lib.y2_detect_anchor_batch_lb(None, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, 416, p, p, p, None) == -1
    assert b"null" in lib.y2_last_error()
    net = buf[:13 * 13 * 5 * 25].view(torch.float32).view(1, 13, 13, 5, 25)
    table = torch.tensor([[0, 375, 500, 1504, 0]], dtype=torch.int64, device="cuda")
    for fn in (E.detect_anchor_batch, E.detect_anchor_classes_batch):
        with pytest.raises(ValueError, match="net_size"):
            fn(net, ANCHORS, table, None, 0.1, 0.5, 10, net_size=448)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


def _snapshot(tmp_path, batch, size):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    model = yolov2.YOLOv2Detector(batch, size, dtype="f32", width_div=8, seed=4)
    for net in model.networks():
        net.load_params(_unit_gain_layers(net))
    weights = str(tmp_path / "unit_gain.npz")
    net_utils.save_yolov2_variables(model, weights, iteration=7)
    return weights


def _forward_of_host_images(detector, host_images):
    """the raw head of `detector` on a list of [size, size, 3] uint8 images (the last one repeated to fill a batch)"""
    import torch
    n = detector.batch
    grids = []
    for lo in range(0, len(host_images), n):
        batch = [host_images[min(k, len(host_images) - 1)] for k in range(lo, lo + n)]
        grids.append(detector.forward(torch.from_numpy(np.stack(batch)).cuda()).clone())
    return torch.cat(grids)[:len(host_images)].cpu().numpy()


def _host_rows_lb(grids, anchors, entries, thresh, nms, max_out, size):
    """_host_rows of the stretch test, with the letterbox map"""
    from tensorflow_yolo2_amd import engine as E
    boxes, scores = E.decode_anchors(grids.contiguous(), anchors)
    best, cls = E.class_argmax(scores)
    boxes, best, cls = (t.cpu().numpy() for t in (boxes, best, cls))
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    for k, e in enumerate(entries):
        det, score = DB.anchor_detect(boxes[k], best[k], cls[k], e["shape"][1], e["shape"][0], thresh, nms, max_out,
                                      net_size=size)
        flag = DB.match_image(det, np.asarray(e["objs"], np.float64), e["difficult"], 0.5) if "objs" in e else det[:, 0] * 0
        rows["image"] += [k] * len(det)
        rows["box"] += det[:, :4].tolist()
        rows["class"] += det[:, 4].tolist()
        rows["candidate"] += det[:, 5].tolist()
        rows["score"] += score.tolist()
        rows["flag"] += flag.tolist()
    return rows


def _host_class_rows_lb(grids, anchors, entries, thresh, nms, max_per_class, size):
    from tensorflow_yolo2_amd import engine as E
    boxes, scores = (t.cpu().numpy() for t in E.decode_anchors(grids.contiguous(), anchors))
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    counts = []
    for k, e in enumerate(entries):
        det, score, count = DB.anchor_detect_classes(boxes[k], scores[k], e["shape"][1], e["shape"][0], thresh, nms,
                                                     max_per_class, net_size=size)
        counts.append(count.tolist())
        for c, m in enumerate(count):
            flag = DB.match_image(det[c, :m], np.asarray(e["objs"], np.float64), e["difficult"], 0.5)
            rows["image"] += [k] * int(m)
            rows["box"] += det[c, :m, :4].tolist()
            rows["class"] += det[c, :m, 4].tolist()
            rows["candidate"] += det[c, :m, 5].tolist()
            rows["score"] += score[c, :m].tolist()
            rows["flag"] += flag.tolist()
    return rows, counts


def _assert_result(r, rows, entries):
    for key in rows:
        assert r["rows"][key].tolist() == rows[key], key
    npos = DB.npos_from_objects([o[4] for e in entries for o in e["objs"]], [d for e in entries for d in e["difficult"]])
    want = DB.map_from_flags((np.array(rows["class"]), np.array(rows["score"], np.float32), np.array(rows["flag"])),
                             npos, use_07_metric=False)
    assert (r["mAP"], r["aps"]) == want and sorted(r["aps"]) == sorted(npos)


@gpu
def test_eval_script_letterbox_equals_the_host_composition(tmp_path, golden_dir):
    """3 images at batch 2 (one partial batch), size 224: with --letterbox the batches are letterbox_u8 of the decoded
    files (the kept grids are the forward pass of exactly those images) and rows, flags, APs and mAP are those of
    anchor_detect(net_size=224), match_image and map_from_flags on the kept grids; with --per-class the same through
    anchor_detect_classes; and without --letterbox the script still returns the stretch composition"""
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    size, batch, M = 224, 2, 6
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    weights = _snapshot(tmp_path, batch, size)
    argv = ["--devkit", kit, "--image-set", "trainval", "--size", str(size), "--batch", str(batch), "--dtype", "f32",
            "--width-div", "8", "--weights", weights, "--thresh", "0.02", "--nms", "0.45", "--max-out", "30",
            "--metric", "10", "--keep-grids"]
    r = pascal_eval_yolov2.main(argv + ["--letterbox"])
    entries = r["imdb"].entries
    assert r["restored"] == 7 and tuple(r["grids"].shape) == (3, 7, 7, 5, 25)
    host_images = [PV.letterbox_u8(PV.imread_bgr(e["imname"]), size) for e in entries]
    assert PV.letterbox_geometry(500, 353, size) == (158, 224, 33, 0) and PV.letterbox_geometry(240, 352, size) == (224, 152, 0, 36)
    assert (host_images[0][:, :33] == 127).all() and (host_images[2][:36] == 127).all()                     # bars
    images, valid = r["imdb"].eval_batch(size, 2, letterbox=True)
    assert valid == 1 and np.array_equal(images.cpu().numpy(), np.stack([host_images[2]] * 2))
    grids = _forward_of_host_images(r["detector"], host_images)
    assert np.array_equal(grids.view(np.uint32), r["grids"].cpu().numpy().view(np.uint32))
    rows = _host_rows_lb(r["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30, size)
    assert len(rows["image"]) > 20 and set(rows["image"]) == {0, 1, 2}
    _assert_result(r, rows, entries)
    assert r["count"].tolist() == [rows["image"].count(k) for k in range(3)]
    # --fill reaches the bars
    images0, _ = r["imdb"].eval_batch(size, 0, letterbox=True, fill=3)
    assert np.array_equal(images0.cpu().numpy()[1], PV.letterbox_u8(PV.imread_bgr(entries[1]["imname"]), size, 3))
    # per class
    c = pascal_eval_yolov2.main(argv + ["--letterbox", "--per-class", "--max-per-class", str(M)])
    assert np.array_equal(c["grids"].cpu().numpy().view(np.uint32), grids.view(np.uint32))
    crows, counts = _host_class_rows_lb(c["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, M, size)
    assert len(crows["image"]) > 20 and len(set(crows["class"])) > 1
    _assert_result(c, crows, entries)
    assert c["count"].tolist() == counts and c["saturated"] == sum(m == M for cc in counts for m in cc)
    # the default is the stretch, as before
    d = pascal_eval_yolov2.main(argv)
    assert not np.array_equal(d["grids"].cpu().numpy(), grids)
    srows = _host_rows(d["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30)
    _assert_result(d, srows, entries)
    assert srows["box"] != rows["box"]


@gpu
def test_detect_script_equals_the_host_composition(tmp_path, golden_dir, capsys):
    """the two golden files through pascal_detect_yolov2: the letterboxed rows by default, the stretch rows with
    --stretch, one printed line per row, and --out holds the lines"""
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    size = 224
    weights = _snapshot(tmp_path, 2, size)
    paths = [os.path.join(golden_dir, n) for n in ("testImg2.jpg", "testImg1.jpg")]
    out = str(tmp_path / "rows.txt")
    argv = ["--images"] + paths + ["--size", str(size), "--dtype", "f32", "--width-div", "8", "--weights", weights,
                                   "--thresh", "0.02", "--max-out", "30", "--keep-grids"]
    capsys.readouterr()
    r = pascal_detect_yolov2.main(argv + ["--out", out])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(golden_dir)]
    shapes = [PV.imread_bgr(p).shape[:2] for p in paths]
    assert shapes == [(500, 353), (240, 352)] and r["restored"] == 7
    entries = [{"shape": s} for s in shapes]
    host_images = [PV.letterbox_u8(PV.imread_bgr(p), size) for p in paths]
    grids = _forward_of_host_images(r["detector"], host_images)
    assert np.array_equal(grids.view(np.uint32), r["grids"].cpu().numpy().view(np.uint32))
    rows = _host_rows_lb(r["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30, size)
    want = [(paths[k], PV.CLASSES[c], s) + tuple(b) for k, c, s, b in zip(rows["image"], rows["class"], rows["score"], rows["box"])]
    assert len(want) > 10 and {w[0] for w in want} == set(paths)
    assert r["rows"] == want
    assert printed == ["%s %s %.6f %d %d %d %d" % w for w in want]
    assert open(out).read().splitlines() == printed
    s = pascal_detect_yolov2.main(argv + ["--stretch"])
    srows = _host_rows(s["grids"], yolov2.ANCHORS_VOC, [dict(e, objs=[], difficult=[]) for e in entries], 0.02, 0.45, 30)
    swant = [(paths[k], PV.CLASSES[c], sc) + tuple(b) for k, c, sc, b in zip(srows["image"], srows["class"], srows["score"], srows["box"])]
    assert s["rows"] == swant and swant != want
