"""The host side of the YOLOv2 evaluation and training plumbing: utils/detect_batch.anchor_candidates / anchor_detect
(the specification of y2_detect_anchor_batch), utils/anchors.kmeans_anchors and the snapshot name map
(utils/yolov2_snapshot.py).  No GPU."""
import numpy as np
import pytest

from test_device_voc_host import make_devkit
from tensorflow_yolo2_amd.utils import anchors as A, detect_batch as DB, voc_eval as V, yolov2_snapshot as SN


def _decode_near_objects(entry, rng, extra=12):
    """a decode (boxes cx, cy, w, h relative; best; cls) whose boxes sit on and around the image's objects, with few
    score levels (ties) and some boxes of other classes and places"""
    h, w = entry["shape"]
    boxes, best, cls = [], [], []
    for (x0, y0, x1, y1, c) in entry["objs"]:
        for _ in range(4):
            j = rng.integers(-12, 13, 4) * (rng.random() < 0.75)
            bw, bh = (x1 - x0 + 1 + j[2]) / w, (y1 - y0 + 1 + j[3]) / h
            boxes.append(((x0 + x1) / 2 + j[0]) / w), boxes.append(((y0 + y1) / 2 + j[1]) / h)
            boxes += [bw, bh]
            best.append(rng.integers(1, 20) / 20.0)
            cls.append(c if rng.random() < 0.85 else rng.integers(0, 20))
    for _ in range(extra):
        boxes += rng.uniform(0.05, 0.95, 2).tolist() + rng.uniform(0.05, 0.6, 2).tolist()
        best.append(rng.integers(1, 20) / 20.0)
        cls.append(rng.integers(0, 20))
    return (np.array(boxes, np.float32).reshape(-1, 4), np.array(best, np.float32), np.array(cls, np.int32))


@pytest.mark.parametrize("use_07", (True, False))
def test_anchor_rows_through_flags_equal_voc_map(tmp_path, golden_dir, use_07):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import read_image_set
    import os
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    _index, entries = read_image_set(os.path.join(kit, "VOC2007"), "trainval")
    rng = np.random.default_rng(21)
    cls, score, flag, dets, gts = [], [], [], [], []
    for k, e in enumerate(entries):
        boxes, best, c = _decode_near_objects(e, rng)
        det, s = DB.anchor_detect(boxes, best, c, e["shape"][1], e["shape"][0], 0.1, 0.6, 100)
        assert 5 < len(det) < len(best) and (np.diff(s.astype(np.float64)) <= 0).all()
        f = DB.match_image(det, np.asarray(e["objs"], np.float64), e["difficult"], 0.5)
        cls += det[:, 4].tolist(); score += s.tolist(); flag += f.tolist()
        dets += [(k, int(d[4]), float(sc), float(d[0]), float(d[1]), float(d[2]), float(d[3])) for d, sc in zip(det, s)]
        gts += [(k, int(o[4]), o[0], o[1], o[2], o[3], int(hard)) for o, hard in zip(e["objs"], e["difficult"])]
    npos = DB.npos_from_objects([g[1] for g in gts], [g[6] for g in gts])
    got = DB.map_from_flags((np.array(cls), np.array(score, np.float32), np.array(flag)), npos, use_07)
    want = V.voc_map(dets, gts, num_class=20, iou_thresh=0.5, use_07_metric=use_07)
    assert got == want                                                   # equal as floats, class by class
    assert (np.array(flag) == 1).sum() >= 3 and (np.array(flag) == 0).sum() >= 3 and 0.0 < got[0] < 1.0


def _one(box, best=0.9, cls=1, im_w=100, im_h=60, thresh=0.5):
    valid, out, c, s = DB.anchor_candidates(np.array([box], np.float32), np.array([best], np.float32), [cls], im_w, im_h,
                                            thresh)
    return bool(valid[0]), out[0].tolist()


def test_anchor_candidates_validity_rules():
    assert _one((0.5, 0.5, 0.2, 0.5)) == (True, [41, 16, 60, 45])        # x 50 w 20 -> 40..59; y 30 h 30 -> 15..44; + 1
    assert _one((0.5, 0.5, 0.2, 0.5), best=np.nan) == (False, [0, 0, 0, 0])
    assert _one((0.5, 0.5, 0.2, 0.5), best=0.5)[0] is False              # equal to the threshold is not above it
    with np.errstate(over="ignore"):
        inf_w = np.float32(3.0) * np.exp(np.float32(100.0)) / np.float32(13.0)      # the decode's exp overflow
    assert np.isinf(inf_w) and _one((0.5, 0.5, inf_w, 0.5))[0] is False
    assert _one((0.5, 0.5, 0.2, np.nan))[0] is False
    assert _one((0.5, 0.5, np.float32(1 << 23), 0.5), im_w=128)[0] is False     # the product is 2^30 exactly
    below = np.nextafter(np.float32(1 << 23), np.float32(0))
    assert _one((0.5, 0.5, below, 0.5), im_w=128) == (True, [1, 16, 128, 45])   # just below: a box, cut on both sides
    assert _one((5.0, 0.5, 0.2, 0.5))[0] is False                         # wholly to the right of the image
    assert _one((0.5, -2.0, 0.2, 0.5))[0] is False                        # wholly above
    assert _one((0.5, 0.5, 0.0, 0.5))[0] is False                         # no width: empty
    assert _one((0.05, 0.5, 0.2, 0.5)) == (True, [1, 16, 15, 45])         # cut at the left edge: -5..14 -> 0..14
    assert _one((0.9375, 0.5, 0.2, 0.5)) == (True, [84, 16, 100, 45])     # right: x 93 (93.75) -> 83..102 -> 83..99
    assert _one((0.5, 0.125, 0.2, 0.5)) == (True, [41, 1, 60, 22])        # top: y 7 (7.5) h 30 -> -8..21 -> 0..21
    assert _one((0.5, 0.875, 0.2, 0.5)) == (True, [41, 38, 60, 60])       # bottom: y 52 (52.5) -> 37..66 -> 37..59
    assert _one((0.505, 0.5, 0.215, 0.5)) == (True, [41, 16, 61, 45])     # toward zero: x 50 (50.5), w 21 (21.5) -> 40..60


def test_anchor_detect_orders_ties_by_index_and_walks_by_class():
    boxes = np.array([(0.2, 0.5, 0.2, 0.4), (0.5, 0.5, 0.2, 0.4), (0.8, 0.5, 0.2, 0.4), (0.5, 0.5, 0.2, 0.4),
                      (0.5, 0.5, 0.2, 0.4), (0.51, 0.5, 0.2, 0.4)], np.float32)
    best = np.array([0.7, 0.7, 0.7, 0.9, 0.6, 0.65], np.float32)
    cls = np.array([0, 1, 0, 1, 2, 1])
    det, score = DB.anchor_detect(boxes, best, cls, 100, 60, 0.1, 0.5, 10)
    # 3 first; 0, 1, 2 tie at 0.7 in index order, 1 is 3's box and class: suppressed; 5 overlaps 3 too; 4 is another class
    assert det[:, 5].tolist() == [3, 0, 2, 4] and det.dtype == np.int32 and score.dtype == np.float32
    assert score.tolist() == [np.float32(0.9), np.float32(0.7), np.float32(0.7), np.float32(0.6)]
    assert DB.anchor_detect(boxes, best, cls, 100, 60, 0.1, 1.0, 10)[0][:, 5].tolist() == [3, 0, 1, 2, 5, 4]
    assert DB.anchor_detect(boxes, best, cls, 100, 60, 0.1, 1.0, 2)[0][:, 5].tolist() == [3, 0]
    assert DB.anchor_detect(boxes, best, cls, 100, 60, 0.95, 0.5, 10)[0].shape == (0, 6)
    # grid_detect goes through the same walk
    assert DB.grid_detect.__code__.co_names.count("_greedy_walk") == DB.anchor_detect.__code__.co_names.count("_greedy_walk") == 1


def test_kmeans_anchors_recovers_planted_clusters():
    rng = np.random.default_rng(0)
    centres = np.array([(1.0, 1.5), (2.5, 6.0), (4.0, 3.0), (8.0, 9.0), (11.0, 5.0)])
    wh = np.concatenate([c * rng.uniform(0.93, 1.07, (300, 2)) for c in centres])
    rng.shuffle(wh)
    got = A.kmeans_anchors(wh, k=5, seed=3, iters=100)
    assert got.dtype == np.float32 and got.shape == (5, 2)
    assert (np.diff(got.prod(axis=1)) > 0).all()                          # sorted by area
    want = centres[np.argsort(centres.prod(axis=1))]
    assert np.abs(got / want - 1).max() < 0.02
    assert A.mean_shape_iou(wh, got) > 0.9
    assert np.array_equal(got, A.kmeans_anchors(wh, k=5, seed=3, iters=100))           # deterministic
    for seed in (0, 1, 2):                                                # whatever the first start
        assert np.abs(A.kmeans_anchors(wh[::-1].copy(), k=5, seed=seed) / want - 1).max() < 0.02
    with pytest.raises(ValueError):
        A.kmeans_anchors(wh[:1].repeat(10, axis=0), k=5)
    with pytest.raises(ValueError):
        A.kmeans_anchors(np.array([(1.0, -1.0)] * 8), k=2)
    # the box table's shapes in cells of stride 32 at a size
    boxes = np.zeros((2, 2, 5)); boxes[0, 0] = (11, 21, 111, 71, 3); boxes[1, :2] = [(1, 1, 51, 26, 0), (5, 5, 5, 9, 1)]
    table = np.array([(0, 100, 200, 608, 0), (0, 50, 100, 304, 0)], np.int64)
    got = A.box_table_wh(boxes, np.array([1, 2], np.int32), table, 416)
    assert np.allclose(got, [(0.5 * 13, 0.5 * 13), (0.5 * 13, 0.5 * 13)])       # the box without width is left out


def test_snapshot_name_map_round_trips():
    rng = np.random.default_rng(5)
    layer = lambda co: {"W": rng.normal(size=(3, 3, 4, co)).astype(np.float32),
                        **{k: rng.normal(size=co).astype(np.float32) for k in ("b", "gamma", "beta", "moving_mean", "moving_var")}}
    stacks = {"stem": [layer(8), layer(4)], "deep": [layer(6)], "head": [layer(2), layer(3), layer(5)]}
    slots = lambda s: [{k: rng.normal(size=l[k].shape).astype(np.float32) for k in SN.PARAM_KEYS} for l in stacks[s]]
    adam = {s: {"m": slots(s), "v": slots(s), "t": 7 + i} for i, s in enumerate(SN.STACKS)}
    scaler = {"ctrl": np.arange(8, dtype=np.int32), "scale": 512.0, "clean": 41}
    anchors = [(1.5, 2.0), (3.0, 4.5)]
    blob = SN.to_blob(stacks, anchors, 20, 1234, adam, scaler)
    assert "yolov2/stem/1/moving_var" in blob and "yolov2/head/2/gamma/Adam_1" in blob and "yolov2/deep/adam_step" in blob
    assert all(isinstance(v, (np.ndarray, np.generic)) for v in blob.values())
    s2, an2, nc2, it2, adam2, scaler2 = SN.from_blob(blob)
    assert (nc2, it2) == (20, 1234) and np.array_equal(an2, np.array(anchors, np.float32))
    for s in SN.STACKS:
        assert len(s2[s]) == len(stacks[s]) and adam2[s]["t"] == adam[s]["t"]
        for a, b in zip(s2[s], stacks[s]):
            assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
        for slot in ("m", "v"):
            for a, b in zip(adam2[s][slot], adam[s][slot]):
                assert all(np.array_equal(a[k], b[k]) for k in SN.PARAM_KEYS)
    assert scaler2["scale"] == 512.0 and scaler2["clean"] == 41 and scaler2["ctrl"].tolist() == list(range(8))
    assert SN.meta_from_blob(blob)[1:] == (20, 1234)
    # a detector's snapshot: parameters only
    plain = SN.to_blob(stacks, anchors, 20, 0)
    assert not any(k.endswith("/Adam") or "scaler" in k or "adam_step" in k for k in plain)
    assert SN.from_blob(plain)[4:] == (None, None)
    with pytest.raises(ValueError, match="yolov2/anchors"):
        SN.from_blob({k: v for k, v in blob.items() if k != "yolov2/anchors"})
    with pytest.raises(ValueError, match=r"anchors is \[\[1.5, 2.0\], \[3.0, 4.5\]\], the model has \[\[1.0, 1.0\]\]"):
        SN.check_matches("anchors", "f.npz", an2, np.ones((1, 2), np.float32))
    SN.check_matches("num_class", "f.npz", 20, 20)
