"""utils/detect_batch.py, the host specification of csrc/detect.hip: the decode against oracle/loss_ref.decode_detections,
per-image matching + global curve against utils/voc_eval.voc_map (equal as floats), and the `difficult` flags that
read_image_set now carries.  No GPU."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from oracle import loss_ref as L
from test_device_voc_host import make_devkit
from tensorflow_yolo2_amd.utils import detect_batch as DB, voc_eval as V


@pytest.mark.parametrize("S", (7, 13))
def test_grid_detect_before_nms_is_the_oracle_decode(S):
    """iou_thresh = 1 suppresses nothing (no IoU is > 1) and max_out = S * S * B keeps everything: what is left is
    decode_detections' kept set with detections_from_decode's corners, cut to the image, + 1, in descending score"""
    B, C, im_w, im_h, thresh = 2, 20, 353, 500, 0.3
    rng = np.random.default_rng(100 + S)
    p = rng.uniform(-0.2, 1.0, (S, S, C + 5 * B)).astype(np.float32)
    p[..., C + B:] = rng.uniform(-0.3, 0.9, (S, S, 4 * B))                # x, y offsets and sqrt(w), sqrt(h)
    p[0, 0, C + B + 2] = 0.0                                              # a box of zero width above the threshold
    p[0, 0, C] = 0.9
    p[1, 2, C + B:C + B + 4] = (0.5, 0.5, 1.4, 1.3)                       # larger than the image: cut on every side
    p[1, 2, C] = 0.8
    p[2, 1, C + 1], p[2, 3, C + 1], p[4, 4, C] = 0.77, 0.77, 0.77          # equal scores: ascending candidate index
    p[2, 1, C + B + 4:], p[2, 3, C + B + 4:], p[4, 4, C + B:C + B + 4] = 3 * [(0.5, 0.5, 0.4, 0.4)]
    det, score = DB.grid_detect(p, im_w, im_h, C, B, thresh, 1.0, S * S * B)
    ref = L.decode_detections(p, im_w, im_h, C, S, B, object_thresh=thresh)
    want = {}
    dropped = cut = 0
    for (ulx, uly, w, h, cls, conf, c, r, b) in ref:
        _img, _cls, _conf, x0, y0, x1, y1 = V.detections_from_decode("i", [(ulx, uly, w, h, cls, conf)])[0]
        cx0, cy0, cx1, cy1 = max(x0, 0), max(y0, 0), min(x1, im_w - 1), min(y1, im_h - 1)
        if cx1 < cx0 or cy1 < cy0:
            dropped += 1
            continue
        cut += (cx0, cy0, cx1, cy1) != (x0, y0, x1, y1)
        want[(c * S + r) * B + b] = (cx0 + 1, cy0 + 1, cx1 + 1, cy1 + 1, cls, np.float32(conf))
    assert dropped >= 1 and cut >= 1 and len(want) > S * S // 2
    assert det.dtype == np.int32 and score.dtype == np.float32 and det.shape == (len(want), 6)
    assert sorted(det[:, 5].tolist()) == sorted(want)
    for row, s in zip(det, score):
        assert tuple(row[:5]) == want[row[5]][:5] and s == want[row[5]][5]
    order = sorted(want, key=lambda i: (-float(want[i][5]), i))
    assert det[:, 5].tolist() == order
    assert (np.diff(score.astype(np.float64)) <= 0).all() and (np.diff(score) == 0).sum() >= 2


def test_grid_detect_validity_rules_and_nms():
    S, B, C = 3, 2, 4
    D = C + 5 * B
    p = np.zeros((S, S, D), np.float32)

    def put(cell, b, conf, box, cls):
        row = p.reshape(S * S, D)[cell]
        row[C + b] = conf
        row[C + B + 4 * b:C + B + 4 * b + 4] = box
        row[:C] = 0
        row[cls] = 1
    put(0, 0, 0.9, (0.5, 0.5, 0.5, 0.5), 1)             # A
    put(0, 1, 0.8, (0.5, 0.5, 0.5, 0.5), 1)             # the same box, same cell and class: suppressed by A
    put(1, 0, np.nan, (0.5, 0.5, 0.5, 0.5), 1)          # NaN confidence: not valid
    put(2, 0, 0.7, (np.inf, 0.5, 0.5, 0.5), 2)          # not finite
    put(3, 0, 0.7, (0.5, 0.5, 1e10, 0.5), 2)            # 1e20 * width: beyond 2^30
    put(4, 0, 0.7, (0.5, 0.5, 0.0, 0.5), 2)             # zero width
    put(5, 0, 0.7, (40.0, 0.5, 0.3, 0.3), 2)            # wholly to the right of the image
    put(6, 0, 0.6, (0.5, 0.5, 0.5, 0.5), 3)             # valid
    det, score = DB.grid_detect(p, 90, 60, C, B, 0.1, 0.5, 10)
    assert det[:, 5].tolist() == [0, 12] and score.tolist() == [np.float32(0.9), np.float32(0.6)]
    det, _ = DB.grid_detect(p, 90, 60, C, B, 0.1, 1.0, 10)
    assert det[:, 5].tolist() == [0, 1, 12]
    det, _ = DB.grid_detect(p, 90, 60, C, B, 0.1, 1.0, 2)              # max_out stops the walk
    assert det[:, 5].tolist() == [0, 1]
    assert DB.grid_detect(p, 90, 60, C, B, 0.95, 0.5, 10)[0].shape == (0, 6)


def _random_case(seed=5):
    """about 40 images, 5 classes (class 4 has no ground truth, class 3 no detections), several hundred detections"""
    rng = np.random.default_rng(seed)
    images = []
    for k in range(40):
        m = int(rng.integers(1, 7))
        gt = np.zeros((m, 5))
        for j in range(m):
            x, y = rng.integers(1, 200, 2)
            gt[j] = (x, y, x + rng.integers(10, 120), y + rng.integers(10, 120), rng.integers(0, 4))
        difficult = (rng.random(m) < 0.25).astype(np.uint8)
        dets = []
        for _ in range(0 if k % 9 == 4 else int(rng.integers(4, 16))):
            if rng.random() < 0.6:                                       # near an object, sometimes exactly on it
                g = gt[rng.integers(0, m)]
                j = rng.integers(-6, 7, 4) * (rng.random() < 0.8)
                box, cls = (g[:4] + j).astype(int).tolist(), int(g[4])
            else:
                x, y = rng.integers(1, 250, 2)
                box, cls = [x, y, x + rng.integers(5, 100), y + rng.integers(5, 100)], int(rng.integers(0, 5))
            if cls == 3:
                cls = 0                                                  # class 3: ground truth, never detected
            dets.append(box + [cls, float(np.float32(rng.integers(1, 40) / 40.0))])   # few levels: many equal scores
        images.append([gt, difficult, dets])
    # two detections on one object, and one detection with equal IoU to two objects of its class
    images[0][0] = np.array([[10, 10, 59, 59, 1], [40, 10, 89, 59, 1], [100, 100, 150, 150, 2]], float)
    images[0][1] = np.array([0, 0, 1], np.uint8)
    images[0][2] = [[25, 10, 74, 59, 1, 0.9], [10, 10, 59, 59, 1, 0.5], [11, 10, 59, 59, 1, 0.5],
                    [100, 100, 150, 150, 2, 0.5], [10, 10, 59, 59, 4, 0.5]]
    return images


def _compose(images, use_07):
    """the per-image path: rows in grid_detect's order (descending score, stable), match_image, map_from_flags"""
    cls, score, flag, npos_c, npos_d = [], [], [], [], []
    for gt, difficult, dets in images:
        d = np.array(sorted(dets, key=lambda r: -r[5]), float).reshape(-1, 6)
        f = DB.match_image(d[:, :5].astype(np.int32), gt, difficult, 0.5)
        cls += d[:, 4].astype(int).tolist()
        score += d[:, 5].astype(np.float32).tolist()
        flag += f.tolist()
        npos_c += gt[:, 4].astype(int).tolist()
        npos_d += difficult.tolist()
    rows = (np.array(cls, np.int32), np.array(score, np.float32), np.array(flag, np.int32))
    return DB.map_from_flags(rows, DB.npos_from_objects(npos_c, npos_d), use_07), rows


def _devkit_way(images, use_07):
    dets, gts = [], []
    for k, (gt, difficult, d) in enumerate(images):
        for r in sorted(d, key=lambda r: -r[5]):
            dets.append((k, int(r[4]), float(np.float32(r[5])), r[0], r[1], r[2], r[3]))
        for g, hard in zip(gt, difficult):
            gts.append((k, int(g[4]), g[0], g[1], g[2], g[3], int(hard)))
    return V.voc_map(dets, gts, num_class=5, iou_thresh=0.5, use_07_metric=use_07)


@pytest.mark.parametrize("use_07", (True, False))
def test_per_image_flags_and_global_curve_equal_voc_map(use_07):
    images = _random_case()
    (m, aps), (cls, score, flag) = _compose(images, use_07)
    want_m, want_aps = _devkit_way(images, use_07)
    assert m == want_m and aps == want_aps                              # equal as floats, class by class
    assert sorted(aps) == [0, 1, 2, 3] and aps[3] == 0.0 and 0.0 < m < 1.0
    # the case holds what it is meant to hold
    assert len(cls) > 300 and (flag == 2).sum() > 5 and (flag == 1).sum() > 20 and (flag == 0).sum() > 20
    assert (cls == 4).sum() > 5 and not (cls == 3).any()
    assert any(not d for _g, _h, d in images)
    assert len(set(score.tolist())) < 41                                # equal scores across and within images
    # image 0: equal IoU to two objects -> the first one; an exact duplicate of it; a near duplicate (its best object is
    # the taken one, whatever else is free); a difficult object; a class without ground truth
    assert flag[:5].tolist() == [1, 0, 0, 2, 0]


def test_match_image_threshold_and_empty_inputs():
    gt = np.array([[1, 1, 10, 10, 0], [21, 1, 30, 10, 0]], float)
    # a 10 x 20 detection over a 10 x 10 object: 100 / 200, exactly the threshold (>= passes); 10 x 21: 100 / 210
    det = np.array([[1, 1, 10, 20, 0], [21, 1, 30, 21, 0]], np.int32)
    assert DB.match_image(det, gt, [0, 0], 0.5).tolist() == [1, 0]
    assert DB.match_image(det[:0], gt, [0, 0], 0.5).tolist() == []
    assert DB.match_image(det, np.zeros((0, 5)), [], 0.5).tolist() == [0, 0]
    m, aps = DB.map_from_flags((np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.int32)), {0: 2}, True)
    assert m == 0.0 and aps == {0: 0.0}
    assert DB.map_from_flags(([0], [0.5], [1]), [1, 0, 0], False) == (1.0, {0: 1.0})


def test_read_image_set_carries_difficult(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import CLASSES, read_image_set
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    data = os.path.join(kit, "VOC2007")
    index, entries = read_image_set(data, "trainval")
    assert index == ["000001", "000002", "000003"] and len(entries) == 3
    for name, e in zip(index, entries):
        root = ET.parse(os.path.join(data, "Annotations", name + ".xml")).getroot()
        objs, hard = [], []
        for o in root.findall("object"):
            bb = o.find("bndbox")
            objs.append(tuple(float(bb.find(k).text) for k in ("xmin", "ymin", "xmax", "ymax")) +
                        (CLASSES.index(o.find("name").text.lower().strip()),))
            hard.append(int(o.find("difficult").text) if o.find("difficult") is not None else 0)
        assert sorted(e) == ["difficult", "imname", "objs", "shape"]
        assert e["objs"] == objs and e["difficult"] == hard and len(hard) == len(objs) > 0
        assert e["imname"] == os.path.join(data, "JPEGImages", name + ".jpg")
    assert entries[2]["difficult"] == [0, 0, 1] and entries[2]["shape"] == (240, 352)
    # a missing <difficult> element counts as 0
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import parse_difficult
    assert parse_difficult("<annotation><object><name>cat</name></object><object><difficult>1</difficult></object>"
                           "</annotation>") == [0, 1]
    hard = DV.build_difficult(entries, 5, flipped=True)
    assert hard.dtype == np.uint8 and hard.shape == (6, 5) and hard[2].tolist() == [0, 0, 1, 0, 0]
    assert (hard[3:] == hard[:3]).all()
