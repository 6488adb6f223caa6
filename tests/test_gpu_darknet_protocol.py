"""Darknet's test-time protocol on the device (csrc/darknet_io.hip): y2_letterbox_darknet_batch bit for bit against
pascal_voc.letterbox_darknet, y2_detect_anchor_classes_batch_dk bit for bit against
utils/detect_batch.anchor_detect_classes_darknet fed with the device's own y2_decode_anchors, y2_voc_match_batch_f
against match_image_f, and pascal_eval_yolov2 / pascal_detect_yolov2 --protocol darknet against the host composition of
the three specifications on the same head outputs.  Everything is equality: no tolerance.
tests/test_darknet_protocol_host.py holds what needs no GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import _darknet_ref as D
from test_device_voc_host import make_devkit
from tensorflow_yolo2_amd.img_dataset import pascal_voc as PV
from tensorflow_yolo2_amd.utils import detect_batch as DB

gpu = pytest.mark.gpu
F = np.float32

# (height, width): the quirk pair and its transpose, extents of 1 both ways, pictures smaller than every output, pictures
# larger than every output, a square; the two golden JPEGs follow them in the pool
POOL_SHAPES = ((8, 21), (21, 8), (1, 40), (40, 1), (5, 7), (7, 5), (75, 100), (100, 75), (33, 33))
ODD_ENTRY = 4                                                             # 5 x 7: offset and pitch off 16 bytes
GOLDEN = ("testImg2.jpg", "testImg1.jpg")
ANCHORS = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))
DK_GEOMETRIES = ((1, 2, 3), (2, 5, 3), (3, 5, 20))
SHAPES = ((333, 500), (500, 375), (64, 64))                              # (height, width): wide, tall, square
SCORE_THRESH, IOU_THRESH = 0.005, 0.45


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def pool(golden_dir):
    """(images, pool, table): the hand-made shapes and the two golden JPEGs in DeviceVOC's layout, but entry ODD_ENTRY
    three bytes off its aligned offset with a pitch of 3 w + 2, and a last table row that is EMPTY (None in images)"""
    import torch
    rng = np.random.default_rng(78)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in POOL_SHAPES]
    images += [PV.imread_bgr(os.path.join(golden_dir, n)) for n in GOLDEN]
    rows, total = [], 0
    for k, img in enumerate(images):
        h, w = img.shape[:2]
        pitch = 16 * ((3 * w + 15) // 16)
        off = total
        if k == ODD_ENTRY:
            off, pitch = total + 3, 3 * w + 2
        rows.append((off, h, w, pitch, 0))
        total = 16 * ((off + h * pitch + 15) // 16)
    flat = rng.integers(0, 256, total, dtype=np.uint8)                    # the padding is not zero: it must not be read
    for img, (off, h, w, pitch, _f) in zip(images, rows):
        view = flat[off:off + h * pitch].reshape(h, pitch)
        view[:, :3 * w] = img.reshape(h, 3 * w)
    rows.append((0, 0, 0, 0, 0))
    assert rows[ODD_ENTRY][0] % 16 and rows[ODD_ENTRY][3] % 16
    return images + [None], torch.from_numpy(flat).cuda(), torch.from_numpy(np.array(rows, np.int64)).cuda()


@gpu
@pytest.mark.parametrize("size", (32, 64, 96))
def test_letterbox_darknet_batch_is_bit_equal_to_the_specification(pool, size):
    import torch
    from tensorflow_yolo2_amd import engine as E
    images, dev_pool, table = pool
    want = [PV.letterbox_darknet(img, size) if img is not None else np.full((size, size, 3), 0.5, F) for img in images]
    if size == 64:
        assert PV.letterbox_geometry(8, 21, 64) == (64, 24, 0, 20) and (want[0][43] < 1e-6).all()   # the quirk row
    n = len(images)
    permuted = [int(v) for v in np.random.default_rng(size).permutation(n)] + [n - 1, 0, 0]
    for index in (None, permuted):
        entries = index if index is not None else list(range(n))
        idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
        out = torch.full((len(entries), size, size, 3), float("nan"), dtype=torch.float32, device="cuda")
        got = E.letterbox_darknet_batch(dev_pool, table, idx, len(entries), size, out=out)
        torch.cuda.synchronize()
        assert got is out
        got = got.cpu().numpy()
        assert np.isfinite(got).all()                                     # every value is written
        for k, e in enumerate(entries):
            assert np.array_equal(_bits(got[k]), _bits(want[e])), (size, index is not None, k, e)


@gpu
def test_letterbox_darknet_batch_argument_errors():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    for (n, size), word in (((0, 64), b"n = 0"), ((-1, 64), b"n = -1"), ((1, 0), b"size = 0"), ((1, 48), b"size = 48"),
                            ((1, 68), b"size = 68"), ((1, 1056), b"size = 1056"), ((1, -32), b"size = -32")):
        assert lib.y2_letterbox_darknet_batch(p, p, None, n, size, p, None) == -1, (n, size)
        assert b"y2_letterbox_darknet_batch" in lib.y2_last_error() and word in lib.y2_last_error(), lib.y2_last_error()
    for null in (0, 1, 5):
        a = [p, p, None, 1, 64, p, None]
        a[null] = None
        assert lib.y2_letterbox_darknet_batch(*a) == -1 and b"null" in lib.y2_last_error()
    assert lib.y2_letterbox_darknet_batch(p, p, None, 1, 64, C.c_void_p(buf.data_ptr() + 4), None) == -1
    assert b"aligned" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


# ---- kernel 2
def _table():
    return np.array([(0, h, w, 16 * ((3 * w + 15) // 16), 0) for (h, w) in SHAPES], np.int64)


def _dk_case(S, B, Cn):
    """net [3][S][S][B][5 + Cn] for the slots (wide, tall, square).  Slot 0: candidates 0 and 1 are one row copied -- equal
    scores in every class.  Slot 1: candidate 0 has a NaN objectness, candidate 1 a small sure box at the canvas' left
    edge, inside the left bar of a tall image.  Slot 2: small sure boxes everywhere, more survivors than the cap."""
    rng = np.random.default_rng(3000 + 100 * S + Cn)
    net = rng.normal(0.0, 1.0, (3, S, S, B, 5 + Cn)).astype(F)
    net[..., 2:4] = rng.uniform(-1.0, 0.5, (3, S, S, B, 2))
    net[..., 4] = rng.normal(0.0, 1.5, (3, S, S, B))
    q = net.reshape(3, S * S * B, 5 + Cn)
    q[0, 0, 4:] = 0.0
    q[0, 0, 4:6] = (8.0, 12.0)                                            # class 0, surer than any random candidate
    q[0, 1] = q[0, 0]
    q[1, 0, 4] = np.nan
    q[1, 1, :5] = (-8.0, 0.0, -3.0, -3.0, 4.0)
    q[2, :, 4] = 3.0
    q[2, :, 2:4] = -2.5
    return net


def _check_dk(dev, decoded, B, entries, index, score_thresh, max_per_class):
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
    got = E.detect_anchor_classes_batch_darknet(dev, ANCHORS[:B], table, idx, score_thresh, IOU_THRESH, max_per_class,
                                                out=out, net_size=size)
    torch.cuda.synchronize()
    det, score, count = (t.cpu().numpy() for t in got)
    wants = []
    for k, e in enumerate(entries):
        want = DB.anchor_detect_classes_darknet(boxes[k], scores[k], SHAPES[e][1], SHAPES[e][0], score_thresh, IOU_THRESH,
                                                max_per_class, size)
        assert np.array_equal(count[k], want[2]), (k, count[k], want[2])
        assert np.array_equal(det[k], want[0]), k                         # float corners as bit patterns; unused rows -1
        assert np.array_equal(_bits(score[k]), _bits(want[1])), k
        wants.append(want)
    return wants


@gpu
@pytest.mark.parametrize("S,B,Cn", DK_GEOMETRIES)
def test_detect_anchor_classes_dk_is_bit_equal_to_the_specification(S, B, Cn):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net = _dk_case(S, B, Cn)
    K = S * S * B
    M = 1 if S == 1 else 4
    dev = torch.from_numpy(net).cuda()
    boxes, scores = (t.cpu().numpy() for t in E.decode_anchors(dev, ANCHORS[:B]))
    boxes, scores = boxes.reshape(3, K, 4), scores.reshape(3, K, Cn)
    decoded = (boxes, scores)
    # the inputs meet every rule, on the host: a tie, a NaN, a box in a bar that is kept EMPTY, a saturated class
    with np.errstate(all="ignore"):
        assert (scores[0, 0] == scores[0, 1]).all() and (scores[0, 0] > SCORE_THRESH).any()
        assert np.isnan(scores[1, 0]).all()
    capped = _check_dk(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, M)
    full = _check_dk(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, K)
    assert (capped[2][2] == M).any() and (full[2][2] > M).any()           # the cap is reached, and it cut rows off
    assert not (full[1][0][..., 5] == 0).any()                            # the NaN candidate is in no class
    rows = full[1][0].reshape(-1, 6)
    bar = rows[rows[:, 5] == 1]
    assert len(bar) >= 1                                                  # the bar box passes, in some class
    corners = np.ascontiguousarray(bar[:, :4]).view(F)
    assert (corners[:, 0] == 1.0).all() and (corners[:, 2] < corners[:, 0]).all()   # xmin raised to 1, xmax below it
    assert full[0][0][0, :2, 5].tolist() == [0, 1]                        # the tie leads class 0, lower candidate first
    kept = sum(int(w[2].sum()) for w in full)
    valid = sum(int((np.nan_to_num(scores[k], nan=-1.0) > SCORE_THRESH).sum()) for k in range(3))
    assert 0 < kept <= valid and (S == 1 or kept < valid)                # rows are kept, rows are suppressed
    # an index with other sizes per slot, and thresholds that pass everything / nothing
    _check_dk(dev, decoded, B, (2, 0, 1), (2, 0, 1), SCORE_THRESH, M)
    _check_dk(dev, decoded, B, (1, 1, 0), (1, 1, 0), 0.02, K)
    _check_dk(dev, decoded, B, (0, 1, 2), (0, 1, 2), -1.0, K)
    _check_dk(dev, decoded, B, (0, 1, 2), None, 2.0, M)


@gpu
def test_dk_net_size_that_is_not_32_S_is_an_argument_error():
    import torch
    from tensorflow_yolo2_amd import _lib as L, engine as E
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    name = b"y2_detect_anchor_classes_batch_dk"
    for net_size in (0, -416, 415, 448, 384, 32):                        # S = 13: only 416 will do
        assert lib.y2_detect_anchor_classes_batch_dk(p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, net_size, p, p, p,
                                                     None) == -1
        assert name + b": net_size = %d" % net_size in lib.y2_last_error()
    assert lib.y2_detect_anchor_classes_batch_dk(p, p, p, None, 1, 21, 5, 20, 0.1, 0.5, 10, 672, p, p, p, None) == -1
    assert name + b": S * S * B = 2205" in lib.y2_last_error()
    assert lib.y2_detect_anchor_classes_batch_dk(p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 0, 416, p, p, p, None) == -1
    assert name + b": max_per_class = 0" in lib.y2_last_error()
    assert lib.y2_detect_anchor_classes_batch_dk(p, p, p, None, 0, 13, 5, 20, 0.1, 0.5, 10, 416, p, p, p, None) == -1
    assert name + b": n = 0" in lib.y2_last_error()
    assert lib.y2_detect_anchor_classes_batch_dk(None, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, 416, p, p, p, None) == -1
    assert b"null" in lib.y2_last_error()
    net = buf[:13 * 13 * 5 * 25].view(torch.float32).view(1, 13, 13, 5, 25)
    table = torch.tensor([[0, 375, 500, 1504, 0]], dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="net_size"):
        E.detect_anchor_classes_batch_darknet(net, ANCHORS, table, None, 0.1, 0.5, 10, net_size=448)
    with pytest.raises(ValueError, match="net_size"):
        E.detect_anchor_classes_batch_darknet(net, ANCHORS, table, None, 0.1, 0.5, 10)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


# ---- kernel 3
@gpu
def test_voc_match_batch_f_equals_match_image_f():
    """two images behind an index: float rows on both sides of one half IoU, a taken object, a difficult one, a class
    without objects, an image without rows; the unused rows of det are -1 and their flags come back -1"""
    import torch
    from tensorflow_yolo2_amd import _lib as L, engine as E
    max_obj, max_out = 3, 8
    gt = np.zeros((3, max_obj, 5), np.float64)
    gt[1, :3] = [[10, 10, 50, 50, 0], [100, 100, 150, 150, 0], [10, 10, 50, 50, 1]]
    gt[2, :1] = [[20.0, 30.0, 220.0, 130.0, 4]]
    counts = np.array([0, 3, 1], np.int32)
    difficult = np.zeros((3, max_obj), np.uint8)
    difficult[1, 1] = 1
    rows = [np.array([[10.25, 10.5, 50.0, 49.75, 0], [10.0, 10.0, 50.0, 50.0, 0], [100.5, 100.0, 150.0, 150.0, 0],
                      [10.0, 10.0, 50.0, 29.49, 1], [10.0, 10.0, 50.0, 29.51, 1], [10.0, 10.0, 50.0, 50.0, 2]], F),
            np.array([[20.5, 30.25, 219.75, 79.5, 4], [20.5, 30.25, 219.75, 80.9, 4]], F),
            np.zeros((0, 5), F)]
    index = [1, 2, 0]
    det = np.full((3, max_out, 6), -1, np.int32)
    count = np.zeros(3, np.int32)
    for k, r in enumerate(rows):
        det[k, :len(r), :4] = np.ascontiguousarray(r[:, :4]).view(np.int32)
        det[k, :len(r), 4] = r[:, 4].astype(np.int32)
        det[k, :len(r), 5] = np.arange(len(r))
        count[k] = len(r)
    want = np.full((3, max_out), -1, np.int32)
    for k, e in enumerate(index):
        want[k, :count[k]] = DB.match_image_f(det[k, :count[k]], gt[e, :counts[e]], difficult[e, :counts[e]], 0.5)
    assert want[0, :6].tolist() == [1, 0, 2, 0, 1, 0] and want[1, :2].tolist() == [0, 1]      # both sides of one half
    dev = lambda a: torch.from_numpy(a).cuda()
    flags = E.voc_match_batch_f(dev(det), None, dev(count), dev(gt), dev(counts), dev(difficult),
                                torch.tensor(index, dtype=torch.int32, device="cuda"), 0.5,
                                out=torch.full((3, max_out), 77, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(flags.cpu().numpy(), want)
    # the integer matcher reads the same words as integers: other flags, so the float one is what ran
    ints = E.voc_match_batch(dev(det), None, dev(count), dev(gt), dev(counts), dev(difficult),
                             torch.tensor(index, dtype=torch.int32, device="cuda"), 0.5)
    assert not np.array_equal(ints.cpu().numpy(), want)
    lib = L.load()
    keep = dev(count)
    p = _ptr(keep)
    assert lib.y2_voc_match_batch_f(None, None, p, p, p, p, None, 1, 3, 10, 0.5, p, None) == -1
    assert b"y2_voc_match_batch_f" in lib.y2_last_error() and b"null" in lib.y2_last_error()
    assert lib.y2_voc_match_batch_f(p, None, p, p, p, p, None, 1, 1025, 10, 0.5, p, None) == -1
    assert b"y2_voc_match_batch_f: max_obj = 1025" in lib.y2_last_error()


# ---- end to end
def _weights(directory, batch, size):
    """a random yolov2-voc `.weights` file of 20 classes at width_div 8"""
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    det = yolov2.YOLOv2Detector(batch, size, num_class=20, dtype="f32", width_div=8, topology="darknet")
    path = str(directory / "narrow_voc.weights")
    DW.write(path, D.random_layers(net_utils.darknet_file_layers(det), 7), 5)
    return path


def _host_rows_dk(grids, anchors, entries, thresh, nms, max_per_class, size):
    """the composition of the three host specifications on kept grids -> (rows, counts per image and class)"""
    from tensorflow_yolo2_amd import engine as E
    boxes, scores = (t.cpu().numpy() for t in E.decode_anchors(grids.contiguous(), anchors))
    n = len(entries)
    boxes, scores = boxes.reshape(n, -1, 4), scores.reshape(n, boxes.size // (4 * n), -1)
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    counts = []
    for k, e in enumerate(entries):
        det, score, count = DB.anchor_detect_classes_darknet(boxes[k], scores[k], e["shape"][1], e["shape"][0], thresh, nms,
                                                             max_per_class, size)
        counts.append(count.tolist())
        for c, m in enumerate(count):
            if "objs" in e:
                flag = DB.match_image_f(det[c, :m], np.asarray(e["objs"], np.float64).reshape(-1, 5), e["difficult"], 0.5)
            else:
                flag = np.zeros(m, np.int32)
            rows["image"] += [k] * int(m)
            rows["box"] += np.ascontiguousarray(det[c, :m, :4]).view(F).tolist()
            rows["class"] += det[c, :m, 4].tolist()
            rows["candidate"] += det[c, :m, 5].tolist()
            rows["score"] += score[c, :m].tolist()
            rows["flag"] += flag.tolist()
    return rows, counts


def _forward_of(detector, host_images):
    import torch
    n = detector.batch
    grids = []
    for lo in range(0, len(host_images), n):
        batch = [host_images[min(k, len(host_images) - 1)] for k in range(lo, lo + n)]
        grids.append(detector.forward(torch.from_numpy(np.stack(batch)).cuda()).clone())
    return torch.cat(grids)[:len(host_images)].cpu().numpy()


@gpu
def test_eval_script_darknet_protocol_equals_the_host_composition(tmp_path, golden_dir):
    """3 images at batch 2 (one partial batch), size 64, f32, a random narrow `.weights` file: the batches are
    letterbox_darknet of the decoded files, the kept grids the forward pass of exactly those, and rows, flags, counts, APs
    and mAP those of anchor_detect_classes_darknet, match_image_f and map_from_flags on the kept grids; the results files
    hold the float rows; and with the switch at its default the evaluator returns what it returns without the argument"""
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    size, batch, M = 64, 2, 6
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    weights = _weights(tmp_path, batch, size)
    results = str(tmp_path / "results")
    argv = ["--devkit", kit, "--image-set", "trainval", "--size", str(size), "--batch", str(batch), "--dtype", "f32",
            "--width-div", "8", "--darknet-weights", weights, "--thresh", "0.005", "--nms", "0.45", "--max-per-class",
            str(M), "--metric", "10", "--keep-grids"]
    r = pascal_eval_yolov2.main(argv + ["--protocol", "darknet", "--results-dir", results])
    entries = r["imdb"].entries
    assert r["detector"].topology == "darknet" and tuple(r["grids"].shape) == (3, 2, 2, 5, 25)
    host_images = [PV.letterbox_darknet(PV.imread_bgr(e["imname"]), size) for e in entries]
    images, valid = r["imdb"].eval_batch(size, 2, protocol="darknet")
    assert valid == 1 and images.dtype.is_floating_point
    assert np.array_equal(_bits(images.cpu().numpy()), _bits(np.stack([host_images[2]] * 2)))
    with pytest.raises(ValueError, match="fill"):
        r["imdb"].eval_batch(size, 0, letterbox=True, fill=3, protocol="darknet")
    grids = _forward_of(r["detector"], host_images)
    assert np.array_equal(_bits(grids), _bits(r["grids"].cpu().numpy()))
    rows, counts = _host_rows_dk(r["grids"], yolov2.ANCHORS_VOC, entries, 0.005, 0.45, M, size)
    assert len(rows["image"]) > 20 and set(rows["image"]) == {0, 1, 2} and len(set(rows["class"])) > 1
    assert r["rows"]["box"].dtype == np.float32
    assert np.array_equal(_bits(r["rows"]["box"]), _bits(np.array(rows["box"], F).reshape(-1, 4)))
    assert np.array_equal(_bits(r["rows"]["score"]), _bits(np.array(rows["score"], F)))
    for key in ("image", "class", "candidate", "flag"):
        assert r["rows"][key].tolist() == rows[key], key
    assert r["count"].tolist() == counts and r["saturated"] == sum(m == M for cc in counts for m in cc)
    npos = DB.npos_from_objects([o[4] for e in entries for o in e["objs"]], [d for e in entries for d in e["difficult"]])
    want = DB.map_from_flags((np.array(rows["class"]), np.array(rows["score"], F), np.array(rows["flag"])), npos,
                             use_07_metric=False)
    assert (r["mAP"], r["aps"]) == want and sorted(r["aps"]) == sorted(npos)
    # the results files: "%f" of the float rows, class by class
    for c, path in enumerate(r["results_files"]):
        lines = ["%s %f %f %f %f %f" % ((r["imdb"].image_index[k], s) + tuple(b))
                 for k, cc, s, b in zip(rows["image"], rows["class"], rows["score"], rows["box"]) if cc == c]
        assert open(path).read().splitlines() == lines
    # the switch is free: at its default the evaluator returns the bits it returns without the argument
    detector, imdb = r["detector"], r["imdb"]
    a = pascal_eval_yolov2.evaluate_yolov2(detector, imdb, size, 0.005, 0.45, 100, False, False, True, M, True, 127)
    b = pascal_eval_yolov2.evaluate_yolov2(detector, imdb, size, 0.005, 0.45, 100, False, False, True, M, True, 127,
                                           protocol="repo")
    assert a["rows"]["box"].dtype == np.int32 and len(a["rows"]["flag"]) > 0
    for key in a["rows"]:
        assert a["rows"][key].dtype == b["rows"][key].dtype and a["rows"][key].tobytes() == b["rows"][key].tobytes(), key
    assert a["mAP"] == b["mAP"] and a["count"].tolist() == b["count"].tolist()
    assert len(a["rows"]["flag"]) != len(rows["flag"]) or a["rows"]["box"].tolist() != rows["box"]
    # refusals: the protocol is per class and letterboxed, and belongs to the darknet topology
    with pytest.raises(ValueError, match="per_class"):
        pascal_eval_yolov2.evaluate_yolov2(detector, imdb, size, per_class=False, letterbox=True, protocol="darknet")
    with pytest.raises(ValueError, match="letterbox"):
        detector.detect_classes_batch(images, imdb.table, imdb.eval_index, protocol="darknet")
    paper = yolov2.YOLOv2Detector(batch, size, dtype="f32", width_div=8)
    with pytest.raises(ValueError, match="paper"):
        paper.detect_classes_batch(images, imdb.table, imdb.eval_index, letterbox=True, protocol="darknet")
    with pytest.raises(ValueError, match="paper"):
        pascal_eval_yolov2.evaluate_yolov2(paper, imdb, size, per_class=True, letterbox=True, protocol="darknet")


@gpu
def test_detect_script_darknet_protocol_prints_the_host_composition(tmp_path, golden_dir, capsys):
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    size = 64
    weights = _weights(tmp_path, 2, size)
    paths = [os.path.join(golden_dir, n) for n in GOLDEN]
    out = str(tmp_path / "rows.txt")
    argv = ["--images"] + paths + ["--size", str(size), "--dtype", "f32", "--width-div", "8", "--darknet-weights", weights,
                                   "--thresh", "0.02", "--max-out", "30", "--keep-grids", "--protocol", "darknet"]
    capsys.readouterr()
    r = pascal_detect_yolov2.main(argv + ["--out", out])
    printed = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith(golden_dir)]
    entries = [{"shape": PV.imread_bgr(p).shape[:2]} for p in paths]
    host_images = [PV.letterbox_darknet(PV.imread_bgr(p), size) for p in paths]
    assert np.array_equal(_bits(_forward_of(r["detector"], host_images)), _bits(r["grids"].cpu().numpy()))
    rows, _counts = _host_rows_dk(r["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30, size)
    want = [(paths[k], PV.CLASSES[c], s) + tuple(b)
            for k, c, s, b in zip(rows["image"], rows["class"], rows["score"], rows["box"])]
    assert len(want) > 4 and {w[0] for w in want} == set(paths)
    assert r["rows"] == want
    assert printed == ["%s %s %f %f %f %f %f" % w for w in want]
    assert open(out).read().splitlines() == printed
