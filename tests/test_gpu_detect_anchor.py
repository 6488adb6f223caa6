"""The YOLOv2 anchor detector from the device pool: y2_detect_anchor_batch (csrc/detect.hip) bit for bit against
utils/detect_batch.anchor_detect fed with the device's own y2_decode_anchors + y2_class_argmax, pascal_eval_yolov2
against the host composition on the same head outputs, and pascal_train_yolov2 with its snapshots.  Everything about the
kernel is equality: no tolerance.  The first test needs no GPU: it checks that the specification alone exercises every
rule on the inputs the GPU test uses."""
import ctypes as C
import os

import numpy as np
import pytest

from test_device_voc_host import make_devkit
from tensorflow_yolo2_amd.utils import detect_batch as DB

gpu = pytest.mark.gpu

ANCHORS = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))
SHAPES = ((333, 500), (500, 375), (240, 352), (97, 150))      # (height, width) of the hand-made table's entries
GEOMETRIES = ((1, 5, 20), (13, 5, 20), (19, 5, 20), (7, 3, 1))   # 5, 845 (one slot per lane), 1805 (two), one class
SCORE_THRESH, IOU_THRESH, MAX_OUT = 0.2, 0.45, 24


def _table():
    return np.array([(0, h, w, 16 * ((3 * w + 15) // 16), 0) for (h, w) in SHAPES], np.int64)


def _anchor_case(S, B, C):
    """(net [3][S][S][B][5 + C], {name: candidate index in image 0}).  Image 0 holds the hand-made candidates on random
    heads, image 1 has nothing above the threshold, image 2 small boxes with high scores: more survivors than MAX_OUT."""
    rng = np.random.default_rng(2000 + 100 * S + C)
    net = rng.normal(0.0, 1.0, (3, S, S, B, 5 + C)).astype(np.float32)
    net[..., 2:4] = rng.uniform(-1.0, 0.5, (3, S, S, B, 2))
    net[..., 4] = rng.normal(-1.0, 1.5, (3, S, S, B))
    net[..., 5:] *= 2.0
    net[1, ..., 4] = -8.0                                                 # image 1: objectness 3e-4
    net[2, ..., 4] = 3.0                                                  # image 2: small boxes, sure of themselves
    net[2, ..., 2:4] = -2.5
    net[2, ..., 5:] *= 3.0
    named = {}
    if S == 1:
        net[0, ..., 4] = 2.0
        return net, named
    q = net[0].reshape(S * S, B, 5 + C)

    def put(name, cell, b, t, cls=None):
        q[cell, b, :5] = t
        if cls is not None:
            q[cell, b, 5:] = 0.0
            q[cell, b, 5 + min(cls, C - 1)] = 8.0
        named[name] = cell * B + b
    mid = (S // 2) * S + S // 2
    put("a", mid, 1, (3, 3, 0, 0, 6), 3)                                  # three boxes a tenth of a cell apart
    put("a_same", mid + 1, 1, (-3, 3, 0, 0, 5), 3)                        # ... the same class: suppressed by a
    put("a_other", mid + S, 1, (3, -3, 0, 0, 5.5), 4)                     # ... another class (where there is one)
    put("nan_to", S, 0, (0, 0, 0, 0, np.nan), 2)
    put("inf_width", S + 1, 0, (0, 0, 100, 0, 6), 2)                      # expf(100) = inf
    put("huge_height", S + 2, 0, (0, 0, 0, 40, 6), 2)                     # 2.4e17 cells: finite, beyond 2^30 pixels
    put("no_width", S + 3, 0, (0, 0, -110, 0, 6), 2)                      # expf(-110) = 0: an empty box
    put("left_top", 0, 1, (-6, -6, 0, 0, 4), 5)
    put("right_bottom", S * S - 1, 1, (6, 6, 0, 0, 4), 6)
    for k in range(6):                                                    # one row copied: equal scores, boxes apart
        q[(S - 2) * S + k, 2] = q[(S - 2) * S, 2] if k else np.concatenate([[0, 0, -1.5, -1.5, 2], q[(S - 2) * S, 2, 5:]])
        named["run%d" % k] = ((S - 2) * S + k) * B + 2
    return net, named


def _spec_rows(decoded, entries, score_thresh, iou_thresh, max_out):
    boxes, best, cls = decoded
    return [DB.anchor_detect(boxes[k], best[k], cls[k], SHAPES[e][1], SHAPES[e][0], score_thresh, iou_thresh, max_out)
            for k, e in enumerate(entries)]


@pytest.mark.parametrize("S,B,C", [g for g in GEOMETRIES if g[0] > 1])
def test_detect_anchor_inputs_exercise_every_rule(S, B, C):
    """no GPU: with the oracle's float32 decode in front, the specification alone keeps, suppresses, drops for every
    reason, cuts at the edges, meets equal scores and runs out of max_out on these inputs"""
    from oracle import ext_ref as X
    net, named = _anchor_case(S, B, C)
    K = S * S * B
    assert K not in (64, 128, 256, 512, 1024, 2048)
    boxes, scores = X.decode_anchors(net, ANCHORS[:B])
    with np.errstate(all="ignore"):
        best, cls = scores.max(axis=2), scores.argmax(axis=2)
    h, w = SHAPES[0]
    valid, box, _cls, score = DB.anchor_candidates(boxes[0], best[0], cls[0], w, h, SCORE_THRESH)
    assert np.isnan(score[named["nan_to"]]) and np.isinf(boxes[0][named["inf_width"], 2])
    assert np.isfinite(boxes[0][named["huge_height"]]).all() and boxes[0][named["no_width"], 2] == 0
    for name in ("nan_to", "inf_width", "huge_height", "no_width"):
        assert not valid[named[name]], name
        assert name == "nan_to" or score[named[name]] > SCORE_THRESH
    for name in ("a", "a_same", "a_other", "left_top", "right_bottom", "run0", "run5"):
        assert valid[named[name]], name
    assert box[named["left_top"]][:2].tolist() == [1, 1] and box[named["right_bottom"]][2:].tolist() == [w, h]
    full, fscore = DB.anchor_detect(boxes[0], best[0], cls[0], w, h, SCORE_THRESH, IOU_THRESH, K)
    kept = full[:, 5].tolist()
    assert 0 < len(kept) < valid.sum()                                    # rows are kept, rows are suppressed
    assert named["a"] in kept and named["a_same"] not in kept
    assert C == 1 or named["a_other"] in kept
    runs = [named["run%d" % k] for k in range(6)]
    assert len({score[i].tobytes() for i in runs}) == 1
    assert [i for i in kept if i in runs] == sorted(i for i in kept if i in runs) and len([i for i in kept if i in runs]) > 1
    counts = [len(d) for d, _s in _spec_rows((boxes, best, cls), (0, 1, 2), SCORE_THRESH, IOU_THRESH, MAX_OUT)]
    assert counts[1] == 0 and counts[2] == MAX_OUT
    assert len(DB.anchor_detect(boxes[2], best[2], cls[2], SHAPES[2][1], SHAPES[2][0], SCORE_THRESH, IOU_THRESH, K)[0]) > MAX_OUT


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _check_anchor(dev, decoded, B, entries, index, score_thresh, iou_thresh, max_out):
    import torch
    from tensorflow_yolo2_amd import engine as E
    table = torch.from_numpy(_table()).cuda()
    idx = torch.tensor(index, dtype=torch.int32, device="cuda") if index is not None else None
    n = len(entries)
    out = (torch.full((n, max_out, 6), 77, dtype=torch.int32, device="cuda"),
           torch.full((n, max_out), 7.0, dtype=torch.float32, device="cuda"),
           torch.full((n,), 77, dtype=torch.int32, device="cuda"))
    det, score, count = E.detect_anchor_batch(dev, ANCHORS[:B], table, idx, score_thresh, iou_thresh, max_out, out=out)
    torch.cuda.synchronize()
    det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    for k, (want_det, want_score) in enumerate(_spec_rows(decoded, entries, score_thresh, iou_thresh, max_out)):
        c = len(want_det)
        assert count[k] == c, (k, count[k], c)
        assert np.array_equal(det[k, :c], want_det), k
        assert np.array_equal(score[k, :c].view(np.uint32), want_score.view(np.uint32)), k
        assert (det[k, c:] == -1).all() and (score[k, c:] == 0).all()
    return count


@gpu
@pytest.mark.parametrize("S,B,C", GEOMETRIES)
def test_detect_anchor_is_bit_equal_to_the_specification(S, B, C):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, _named = _anchor_case(S, B, C)
    K = S * S * B
    dev = torch.from_numpy(net).cuda()
    boxes, scores = E.decode_anchors(dev, ANCHORS[:B])
    best, cls = E.class_argmax(scores)
    decoded = tuple(t.cpu().numpy() for t in (boxes, best, cls))
    count = _check_anchor(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, IOU_THRESH, MAX_OUT)
    if S > 1:
        assert count.tolist()[1:] == [0, MAX_OUT] and 0 < count[0] <= MAX_OUT
    _check_anchor(dev, decoded, B, (3, 1, 1), (3, 1, 1), SCORE_THRESH, IOU_THRESH, MAX_OUT)    # an index, other sizes
    full = _check_anchor(dev, decoded, B, (2, 0, 3), (2, 0, 3), SCORE_THRESH, IOU_THRESH, K)   # max_out cuts nothing off
    assert S == 1 or full[2] > MAX_OUT
    _check_anchor(dev, decoded, B, (0, 1, 2), None, SCORE_THRESH, 1.0, K)                      # nothing suppressed
    _check_anchor(dev, decoded, B, (0, 1, 2), (0, 1, 2), -1.0, 0.0, K)           # every score passes, every overlap goes


@gpu
def test_detect_anchor_argument_errors():
    import torch
    from tensorflow_yolo2_amd import _lib as L
    lib = L.load()
    buf = torch.full((1 << 16,), 5, dtype=torch.int32, device="cuda")
    p = _ptr(buf)
    before = buf.clone()
    #           n  S   B     C  max_out
    for case in ((1, 1, 2049, 20, 10), (1, 21, 5, 20, 10), (1, 13, 17, 20, 10), (1, 13, 5, 0, 10), (0, 13, 5, 20, 10),
                 (1, 13, 5, 20, 0)):
        n, S, B, ncls, max_out = case
        assert lib.y2_detect_anchor_batch(p, p, p, None, n, S, B, ncls, 0.1, 0.5, max_out, p, p, p, None) == -1, case
        assert b"y2_detect_anchor_batch" in lib.y2_last_error()
    assert b"max_out" in lib.y2_last_error()
    for null in (0, 1, 2, 11, 12, 13):
        a = [p, p, p, None, 1, 13, 5, 20, 0.1, 0.5, 10, p, p, p, None]
        a[null] = None
        assert lib.y2_detect_anchor_batch(*a) == -1 and b"null" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)                                       # nothing was launched


def _unit_gain_layers(net):
    """the initial filters (standard deviation 0.1) with a batch-norm scale that keeps activations of order 1 on the
    initial moving statistics (mean 0, variance 1): the head then gives finite boxes and scores that vary"""
    layers = net.export_params()
    for layer, (k, ci, _co, _p) in zip(layers, net.spec):
        layer["gamma"][:] = 1.0 / (0.1 * np.sqrt(k * k * ci) * 0.71)
    return layers


def _host_rows(grids, anchors, entries, thresh, nms, max_out):
    import torch
    from tensorflow_yolo2_amd import engine as E
    boxes, scores = E.decode_anchors(grids.contiguous(), anchors)
    best, cls = E.class_argmax(scores)
    boxes, best, cls = (t.cpu().numpy() for t in (boxes, best, cls))
    rows = {k: [] for k in ("image", "box", "class", "candidate", "score", "flag")}
    for k, e in enumerate(entries):
        det, score = DB.anchor_detect(boxes[k], best[k], cls[k], e["shape"][1], e["shape"][0], thresh, nms, max_out)
        flag = DB.match_image(det, np.asarray(e["objs"], np.float64), e["difficult"], 0.5)
        rows["image"] += [k] * len(det)
        rows["box"] += det[:, :4].tolist()
        rows["class"] += det[:, 4].tolist()
        rows["candidate"] += det[:, 5].tolist()
        rows["score"] += score.tolist()
        rows["flag"] += flag.tolist()
    return rows


@gpu
@pytest.mark.parametrize("size,batch,dtype", ((224, 2, "f32"), (608, 1, "f16")))
def test_eval_script_equals_the_host_composition(tmp_path, golden_dir, capsys, size, batch, dtype):
    """3 images (at batch 2: one partial batch) through a detector restored from a snapshot: rows, flags and APs are
    those of anchor_detect, match_image and map_from_flags on the SAME head outputs.  608 is the two-slot path (1805
    candidates) through the whole script; it runs in f16 because the width_div = 8 stem has a 3 x 3 layer 32 -> 32 at
    152 x 152 (104 x 104 at 416) that the f32 inference convolution refuses (launch_conv: invalid argument; the full-width
    model has no such layer, and 224 is below it) -- the comparison is equality on the kept grids either way."""
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import CLASSES
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    model = yolov2.YOLOv2Detector(batch, size, dtype=dtype, width_div=8, seed=4)
    for net in model.networks():
        net.load_params(_unit_gain_layers(net))
    weights = str(tmp_path / "unit_gain.npz")
    net_utils.save_yolov2_variables(model, weights, iteration=7)
    del model
    r = pascal_eval_yolov2.main(["--devkit", kit, "--image-set", "trainval", "--size", str(size), "--batch", str(batch),
                                 "--dtype", dtype, "--width-div", "8", "--weights", weights, "--thresh", "0.02",
                                 "--nms", "0.45", "--max-out", "30", "--metric", "10", "--keep-grids"])
    S = size // 32
    assert r["restored"] == 7 and tuple(r["grids"].shape) == (3, S, S, 5, 25)
    assert np.isfinite(r["grids"].cpu().numpy()).all()
    entries = r["imdb"].entries
    rows = _host_rows(r["grids"], yolov2.ANCHORS_VOC, entries, 0.02, 0.45, 30)
    assert len(rows["image"]) > 20 and set(rows["image"]) == {0, 1, 2}       # detections exist in every image
    for key in rows:
        assert r["rows"][key].tolist() == rows[key], key
    assert r["count"].tolist() == [rows["image"].count(k) for k in range(3)]
    npos = DB.npos_from_objects([o[4] for e in entries for o in e["objs"]], [d for e in entries for d in e["difficult"]])
    assert r["npos"] == npos and npos[CLASSES.index("bird")] == 0
    want = DB.map_from_flags((np.array(rows["class"]), np.array(rows["score"], np.float32), np.array(rows["flag"])),
                             npos, use_07_metric=False)
    assert (r["mAP"], r["aps"]) == want and sorted(r["aps"]) == sorted(npos)
    out = capsys.readouterr().out
    assert "Mean AP = %.4f" % want[0] in out and "AP for bird = 0.0000" in out


def _train(kit, ckpt, iters, dtype, extra=()):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2
    return pascal_train_yolov2.main(["--devkit", kit, "--iters", str(iters), "--batch", "2", "--size", "224", "--dtype",
                                     dtype, "--width-div", "8", "--ckpt-dir", ckpt] + list(extra))


def _largest_difference(a, b):
    """largest |a - b| over every array of two snapshots (exact words compare as numbers too); keys must agree"""
    assert sorted(a.files) == sorted(b.files)
    worst = 0.0
    for k in a.files:
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        assert x.shape == y.shape, k
        if x.size and not np.array_equal(a[k], b[k]):
            worst = max(worst, float(np.nanmax(np.abs(x - y))))
    return worst


@gpu
@pytest.mark.parametrize("dtype", ("f32", "f16"))
def test_resumed_training_continues_the_uninterrupted_run(tmp_path, golden_dir, dtype):
    """5 iterations in one run against 3, a snapshot, a fresh trainer from --ckpt-dir and 2 more: parameters, batch-norm
    state, the Adam moments and the loss scaler (f16).  The control is a second uninterrupted run: where it is bitwise
    equal to the first, so must the resumed run be; else the resumed run may differ by twice the control's difference."""
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    dirs = [str(tmp_path / d) for d in ("whole", "control", "resumed")]
    whole = _train(kit, dirs[0], 5, dtype)
    _train(kit, dirs[1], 5, dtype)
    first = _train(kit, dirs[2], 3, dtype)
    second = _train(kit, dirs[2], 2, dtype)
    assert (first["first_iter"], first["last_iter"], second["first_iter"], second["last_iter"]) == (1, 3, 4, 5)
    assert second["trainer"] is not first["trainer"] and second["trainer"].iteration == 5
    losses = np.array(whole["losses"])
    assert losses.shape == (5, 5) and np.isfinite(losses).all()
    snaps = [np.load(os.path.join(d, "train_iter_5.npz")) for d in dirs]
    assert int(snaps[2]["yolov2/iteration"]) == 5 and int(snaps[2]["yolov2/stem/adam_step"]) == int(snaps[0]["yolov2/stem/adam_step"])
    assert ("yolov2/scaler/ctrl" in snaps[0].files) == (dtype == "f16")
    assert np.abs(snaps[0]["yolov2/head/1/W/Adam_1"]).max() > 0
    control = _largest_difference(snaps[0], snaps[1])
    resumed = _largest_difference(snaps[0], snaps[2])
    print("yolov2 resume %s: control run-to-run difference %.3e, resumed difference %.3e" % (dtype, control, resumed))
    if control == 0.0:
        assert resumed == 0.0
        assert np.array_equal(np.array(first["losses"] + second["losses"]).view(np.uint32), losses.view(np.uint32))
    else:
        assert resumed <= 2.0 * control


@gpu
def test_snapshot_restores_into_a_detector_and_backbone_loader(tmp_path, golden_dir):
    import torch
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    r = _train(kit, str(tmp_path / "ckpt"), 2, "f32")
    snapshot = os.path.join(str(tmp_path / "ckpt"), "train_iter_2.npz")
    trainer = r["trainer"]
    restored = yolov2.YOLOv2Detector(2, 224, dtype="f32", width_div=8, seed=11)
    by_hand = yolov2.YOLOv2Detector(2, 224, dtype="f32", width_div=8, seed=12)
    assert net_utils.restore_yolov2_variables(restored, snapshot) == 2 and restored.iteration == 2
    for src, dst in zip(trainer.networks(), by_hand.networks()):
        dst.load_params(src.export_params())
    images = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 224, 224, 3), dtype=np.uint8)).cuda()
    a, b = restored.forward(images).cpu().numpy(), by_hand.forward(images).cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # another class count, other anchors, another width: each names both values
    with pytest.raises(ValueError, match=r"num_class is 20, the model has 3"):
        net_utils.restore_yolov2_variables(yolov2.YOLOv2Detector(2, 224, num_class=3, dtype="f32", width_div=8), snapshot)
    with pytest.raises(ValueError, match=r"anchors is \[\[.*the model has \[\["):
        net_utils.restore_yolov2_variables(
            yolov2.YOLOv2Detector(2, 224, anchors=[(1, 1)] * 5, dtype="f32", width_div=8), snapshot)
    with pytest.raises(ValueError, match=r"yolov2/stem/5/W has shape \(3, 3, 32, 32\), the model expects \(3, 3, 32, 64\)"):
        net_utils.restore_yolov2_variables(yolov2.YOLOv2Detector(2, 224, dtype="f32", width_div=4), snapshot)
    # the 18 core layers of a Darknet-19 snapshot: 0-12 -> stem, 13-17 -> the first five of the 13 x 13 stack
    sa, sb, _sc = yolov2.yolov2_specs(20, 5, 8)
    rng = np.random.default_rng(8)
    core = []
    for (k, ci, co, _p) in sa + sb[:5]:
        core.append({"W": rng.normal(0, 0.1, (k, k, ci, co)).astype(np.float32),
                     **{key: rng.normal(1, 0.1, co).astype(np.float32)
                        for key in ("b", "gamma", "beta", "moving_mean", "moving_var")}})
    before = [net.export_params() for net in by_hand.networks()]
    assert net_utils.load_darknet19_backbone(by_hand, core + [core[-1]]) == 18       # a classifier's 19th layer is cut
    stem, deep, head = [net.export_params() for net in by_hand.networks()]
    assert len(stem) == 13 and np.array_equal(stem[12]["W"], core[12]["W"]) and np.array_equal(stem[0]["beta"], core[0]["beta"])
    assert np.array_equal(deep[0]["W"], core[13]["W"]) and np.array_equal(deep[4]["moving_var"], core[17]["moving_var"])
    assert np.array_equal(deep[5]["W"], before[1][5]["W"]) and np.array_equal(head[0]["W"], before[2][0]["W"])
    with pytest.raises(ValueError, match="18"):
        net_utils.load_darknet19_backbone(by_hand, core[:17])


@gpu
def test_train_script_multi_scale_and_augmentation(tmp_path, golden_dir):
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    r = _train(kit, str(tmp_path / "ckpt"), 4, "f16", ("--multi-scale", "--ms-sizes", "224,256", "--ms-period", "1",
                                                       "--augment", "--anchors", "kmeans"))
    from tensorflow_yolo2_amd.trainer import multi_scale_size
    assert r["sizes"] == [multi_scale_size(i, (224, 256), 1) for i in range(1, 5)] and set(r["sizes"]) == {224, 256}
    assert np.isfinite(np.array(r["losses"])).all() and len(r["losses"]) == 4
    assert r["anchors"].shape == (5, 2) and (np.diff(r["anchors"].prod(axis=1)) >= 0).all()
    assert os.path.isfile(os.path.join(str(tmp_path / "ckpt"), "train_iter_4.npz"))
