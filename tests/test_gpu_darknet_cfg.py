"""Models built from Darknet cfg files on the GPU (yolo2_nets/yolov2.py from_cfg; utils/darknet_cfg.py; the cfgs of
tests/golden/cfg, written by hand for this repository):

  1. identity   a cfg that describes the "darknet" / "tiny" graph at the widths of width_div = 8 gives the named topology's
                model: bit-equal forward outputs at 64 and 96 from one random `.weights` file, the file's bytes back from
                save_darknet_weights, a float-count error that names the cfg's count and the file's
  2. new ground a chain whose last-but-one convolution narrows (the yolov2-tiny.cfg shape) and a passthrough with a
                32-wide route convolution, 7 classes and 3 anchors, against the float64 restatements of
                tests/_darknet_tiny_ref.py and tests/_darknet_ref.py under the whole-model gate max |d| < 1e-3 max |ref|;
                the detections use the cfg's anchors
  3. training   YOLOv2DarknetTrainer.from_cfg on both, f32 and f16: two finite steps, the padding of a 16-filter first
                layer still bit-zero, the snapshot reloads into YOLOv2Detector.from_cfg, the solver is the record's
  4. callers    train / evaluate / detect with --cfg (and --names), the recipe line, flag-over-file precedence, the
                argument errors"""
import os

import numpy as np
import pytest

import _darknet_ref as R
import _darknet_tiny_ref as T

gpu = pytest.mark.gpu
BATCH = 2
NAMED = {"narrow-darknet.cfg": "darknet", "narrow-tiny.cfg": "tiny"}
NEW = {"chain-narrowing.cfg": "tiny", "passthrough-route32.cfg": "darknet"}
BARE = "passthrough-bare-route.cfg"          # the first-release layout: the route has no convolution


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def record(golden_dir, name):
    from tensorflow_yolo2_amd.utils import darknet_cfg
    return darknet_cfg.load(os.path.join(golden_dir, "cfg", name))


_FILES = {}


def weights_file(tmp_path_factory, golden_dir, name, seed=2026, seen=64000):
    """(path, record, the arrays) of one random `.weights` file of a cfg, written once per session"""
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    if name not in _FILES:
        rec = record(golden_dir, name)
        layers = R.random_layers(rec.file_layers, seed)
        path = str(tmp_path_factory.mktemp("cfg") / (name.replace(".cfg", ".weights")))
        DW.write(path, layers, seen)
        _FILES[name] = (path, rec, layers)
    return _FILES[name]


def images(size):
    return np.random.default_rng(size).integers(0, 256, (BATCH, size, size, 3), dtype=np.uint8)


def bare_route_forward(layers, x):
    """tests/_darknet_ref.yolov2_voc_forward without the route convolution: the fine map itself is reorganised"""
    from tensorflow_yolo2_amd.utils.darknet_reorg import reorg_darknet_chw
    assert len(layers) == 22
    for l in range(13):
        x = R.conv_layer(x, layers[l])
        if l in R.POOL_AFTER:
            x = R.maxpool_chw(x)
    fine = x
    x = R.maxpool_chw(fine)
    for l in range(13, 20):
        x = R.conv_layer(x, layers[l])
    x = np.concatenate([reorg_darknet_chw(fine), x], axis=0)
    return R.conv_layer(R.conv_layer(x, layers[20]), layers[21], leaky=False)


def reference_forward(name, layers, images_u8):
    f = {BARE: bare_route_forward, "chain-narrowing.cfg": T.tiny_forward}.get(name, R.yolov2_voc_forward)
    return np.stack([f(layers, (img[:, :, ::-1].astype(np.float64) / 255.0).transpose(2, 0, 1)).transpose(1, 2, 0)
                     for img in images_u8])


# ---------------------------------------------------------------- 1. identity with the named topologies
@gpu
@pytest.mark.parametrize("name", sorted(NAMED))
def test_cfg_of_a_named_graph_is_the_named_topology(tmp_path_factory, tmp_path, golden_dir, name):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    path, rec, layers = weights_file(tmp_path_factory, golden_dir, name)
    topology = NAMED[name]
    for size in (64, 96):
        cfg = yolov2.YOLOv2Detector.from_cfg(rec, BATCH, size, dtype="f32")
        named = yolov2.YOLOv2Detector(BATCH, size, num_class=3, anchors=yolov2._TOPOLOGY[topology].anchors, dtype="f32",
                                      width_div=8, topology=topology)
        assert cfg.topology == topology and cfg.cfg is rec and cfg.num_class == 3 and cfg.B == 5 and cfg.bn_eps == 1e-6
        np.testing.assert_array_equal(cfg.anchors, named.anchors)
        assert len(cfg.networks()) == len(named.networks())
        for a, b in zip(cfg.networks(), named.networks()):
            assert [tuple(l) for l in a.spec] == [tuple(l) for l in b.spec] and a.core_layers == b.core_layers
            assert (a.slopes is None and b.slopes is None) or list(a.slopes) == list(b.slopes)
        assert net_utils.darknet_file_layers(cfg) == net_utils.darknet_file_layers(named) == list(rec.file_layers)
        assert net_utils.load_darknet_weights(cfg, path) == net_utils.load_darknet_weights(named, path) == 64000
        x = dev(images(size))
        got, want = host(cfg.forward(x)), host(named.forward(x))
        assert got.shape == (BATCH, size // 32, size // 32, 5, 8) and np.abs(want).max() > 0
        assert got.tobytes() == want.tobytes()
    back = str(tmp_path / "back.weights")
    net_utils.save_darknet_weights(cfg, back, 64000)
    assert open(back, "rb").read() == open(path, "rb").read()
    # the training contexts are the named trainer's too
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(rec, dtype="f32")
    named_tr = yolov2.YOLOv2DarknetTrainer(BATCH, 64, num_class=3, dtype="f32", width_div=8, topology=topology)
    assert tr.batch == rec.batch == BATCH and tr.default_size == rec.size == 64 and tr.cf == named_tr.cf
    for a, b in zip(tr.networks(), named_tr.networks()):
        assert [tuple(l) for l in a.spec] == [tuple(l) for l in b.spec] and a.core_layers == b.core_layers
    assert tr._topo.pool is named_tr._topo.pool and tr._topo.concat is named_tr._topo.concat
    assert tr._topo.centre_tap == named_tr._topo.centre_tap and tuple(tr._topo.narrow) == tuple(named_tr._topo.narrow)
    # a file of another float count: the error names the cfg, its count and the file's
    short = str(tmp_path / "short.weights")
    DW.write(short, layers[:-1] + [dict(layers[-1], weights=layers[-1]["weights"][:-1], biases=layers[-1]["biases"][:-1])], 1)
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_weights(cfg, short)
    msg = str(e.value)
    assert rec.path in msg and str(rec.floats) in msg and str(DW.read(short)[4].size) in msg and short in msg


# ---------------------------------------------------------------- 2. new ground, forward
@gpu
@pytest.mark.parametrize("size", [64, 96])
@pytest.mark.parametrize("name", sorted(NEW) + [BARE])
def test_new_graphs_match_darknet_arithmetic(tmp_path_factory, golden_dir, name, size):
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    path, rec, layers = weights_file(tmp_path_factory, golden_dir, name, seed=77)
    det = yolov2.YOLOv2Detector.from_cfg(rec.path, BATCH, size, dtype="f32")          # from the file's path
    assert det.topology == NEW.get(name, "darknet") and det.num_class == 7 and det.B == 3 and rec.classes == 7 and rec.num == 3
    assert net_utils.load_darknet_weights(det, path) == 64000
    x = images(size)
    grid = host(det.forward(dev(x)))
    S = size // 32
    assert grid.shape == (BATCH, S, S, 3, 12) and len(det.networks()) == {"tiny": 2, "darknet": 3 if name == BARE else 4}[
        det.topology]
    ref = reference_forward(name, layers, x).reshape(grid.shape)
    err = np.abs(grid - ref).max() / np.abs(ref).max()
    print("%s, f32, size %d: max |d| / max |ref| = %.3e (max |ref| %.3f)" % (name, size, err, np.abs(ref).max()))
    assert err < 1e-3
    if name == "chain-narrowing.cfg":
        # the detections decode with the cfg's anchors, not with a named graph's
        assert det.head.spec[-2][2] < det.head.spec[-3][2]    # the last-but-one convolution narrows
        boxes = host(det.detect(dev(x))[0])
        g = dev(grid)
        with_cfg = host(E.decode_anchors(g, rec.anchors)[0])
        with_tiny = host(E.decode_anchors(g, yolov2.ANCHORS_TINY_VOC[:3])[0])
        assert boxes.tobytes() == with_cfg.tobytes() and not np.array_equal(with_cfg, with_tiny)


# ---------------------------------------------------------------- 3. training from a cfg
def two_objects(size, num_class):
    truth = np.zeros((BATCH, 30, 5), np.float32)
    u = size / 64.0
    for i in range(BATCH):
        truth[i, 0] = (21.0 * u, 26.0 * u, 23.0 * u, 29.0 * u, i % num_class)
        truth[i, 1] = (44.0 * u, 39.0 * u, 20.0 * u, 18.0 * u, (i + 1) % num_class)
    return dev(truth), dev(np.full(BATCH, 2, np.int32))


@gpu
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", sorted(NEW) + [BARE])
def test_training_from_a_cfg(tmp_path_factory, tmp_path, golden_dir, name, dtype):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    path, rec, _layers = weights_file(tmp_path_factory, golden_dir, name, seed=77)
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(rec, BATCH, 64, dtype=dtype, seed=2)
    assert tr.solver == rec.solver and all(type(o) is E.DarknetSGD for o in tr.opts)
    assert tr.area_weight and tr.prior_images == 12800 and tr.scales == dict(rec.scales) and tr.num_class == 7 and tr.B == 3
    stacks = {"chain-narrowing.cfg": 2, "passthrough-route32.cfg": 4, BARE: 3}[name]
    assert tr.topology == NEW.get(name, "darknet") and len(tr.opts) == len(tr.networks()) == stacks
    assert tr.cf == {2: None, 4: 32, 3: 64}[stacks]           # the width the passthrough reorganises
    net_utils.load_darknet_weights(tr, path)
    narrow = dict(tr._topo.narrow)
    assert narrow == ({0: 16} if name == "chain-narrowing.cfg" else {})
    x = dev(images(64))
    truth, ntruth = two_objects(64, 7)
    start = tr.networks()[0].export_params()
    for it in range(2):
        loss = tr.step(x, truth=truth, ntruth=ntruth)
        assert np.isfinite(host(loss)).all(), it
    torch.cuda.synchronize()
    end = [net.export_params() for net in tr.networks()]
    assert not np.array_equal(end[0][0]["W"][..., :16], start[0]["W"][..., :16])          # the real entries train
    if narrow:                                                # the padding of the 16-filter first layer: still bit-zero
        p0, p1 = end[0][0], end[0][1]
        assert p0["W"].shape[3] == 32 and not p0["W"][..., 16:].any() and not p1["W"][:, :, 16:, :].any()
        assert not p0["b"][16:].any() and not p0["beta"][16:].any() and (p0["gamma"][16:] == 1).all()
    ckpt = str(tmp_path / "ckpt")
    os.makedirs(ckpt)
    snap = net_utils.save_yolov2_snapshot(tr, ckpt, 2)
    assert snap.endswith("train_iter_2.weights") and net_utils.latest_yolov2_snapshot(ckpt, tr.topology) == snap
    det = yolov2.YOLOv2Detector.from_cfg(rec, BATCH, 64, dtype=dtype, seed=7)
    assert net_utils.restore_yolov2_snapshot(det, snap) == 2
    for a_net, b_net in zip(det.networks(), end):
        for a, b in zip(a_net.export_params(), b_net):
            np.testing.assert_array_equal(a["W"], b["W"])
            np.testing.assert_array_equal(a["beta"], b["beta"])
    assert np.isfinite(host(det.forward(x))).all()


# ---------------------------------------------------------------- 4. the callers
def test_train_flags_resolve_against_the_cfg(golden_dir):
    """parse_args alone (no device): what --cfg implies, what a flag overrides, what is refused"""
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as P
    cfg = os.path.join(golden_dir, "cfg", "narrow-tiny.cfg")                      # random=1
    base = ["--devkit", "nowhere", "--cfg", cfg]
    a = P.parse_args(base)
    assert a.topology == "tiny" and a.augment and a.box_labels and a.area_weight and a.prior_images == 12800
    assert a.solver == "darknet" and a.solver_record == a.cfg_record.solver and a.multi_scale
    assert (a.size, a.batch, a.jitter, a.hue, a.saturation, a.exposure) == (64, 2, 0.3, 0.1, 1.5, 1.5)
    b = P.parse_args(base + ["--single-scale", "--jitter", "0.1", "--size", "96", "--batch", "4", "--lr", "0.01",
                             "--prior-images", "64"])
    assert not b.multi_scale and (b.size, b.batch, b.jitter, b.prior_images) == (96, 4, 0.1, 64)
    assert b.augmentation.jitter == 0.1 and b.augmentation.hue == 0.1
    assert float(b.solver_record.learning_rate) == 0.01 and b.solver_record.steps == a.cfg_record.solver.steps
    assert P.parse_args(["--devkit", "nowhere", "--cfg", os.path.join(golden_dir, "cfg", "narrow-darknet.cfg")]).topology == \
        "darknet"
    for extra in (["--topology", "paper"], ["--topology", "darknet"], ["--imagenet-ckpt-dir", "x"], ["--anchors", "kmeans"],
                  ["--width-div", "8"]):
        with pytest.raises(SystemExit):
            P.parse_args(base + extra)
    for argv in (["--devkit", "nowhere", "--region-stats"], ["--devkit", "nowhere", "--single-scale"],
                 ["--devkit", "nowhere", "--cfg", os.path.join(golden_dir, "cfg", "missing.cfg")]):
        with pytest.raises(SystemExit):
            P.parse_args(argv)
    plain = P.parse_args(["--devkit", "nowhere"])               # without --cfg: today's defaults
    assert (plain.size, plain.batch, plain.jitter, plain.hue, plain.saturation, plain.exposure, plain.prior_images,
            plain.anchors, plain.topology, plain.solver_record, plain.augmentation) == \
        (416, 24, 0.3, 0.1, 1.5, 1.5, 0, "voc", "paper", None, None)


@gpu
def test_callers_take_a_cfg(tmp_path_factory, tmp_path, golden_dir, capsys):
    from test_box_list_host import build_devkit
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2, pascal_eval_yolov2, pascal_train_yolov2
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    name = "narrow-tiny-voc.cfg"                              # 20 classes, random=0, jitter .2
    path, rec, _layers = weights_file(tmp_path_factory, golden_dir, name, seed=9, seen=6)
    cfg = rec.path
    three = os.path.join(golden_dir, "cfg", "narrow-tiny.cfg")
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    ckpt = str(tmp_path / "ckpt")
    train = ["--devkit", kit, "--cfg", cfg, "--dtype", "f32"]
    capsys.readouterr()
    first = pascal_train_yolov2.main(train + ["--darknet-weights", path, "--iters", "10", "--ckpt-dir", ckpt,
                                              "--region-stats"])
    out = capsys.readouterr().out
    assert "cfg recipe: box labels, area weight, prior images 12800, jitter 0.2, hue 0.1" in out
    assert "topology tiny, 20 classes, 5 anchors, size 64, batch 2, multi-scale off" in out and "cfg solver: Solver(" in out
    assert out.count("Region Avg IOU: ") == 1 and ", Avg Recall: " in out and ",  count: " in out
    tr = first["trainer"]
    assert first["topology"] == "tiny" and isinstance(tr, yolov2.YOLOv2DarknetTrainer) and tr.cfg is not None
    assert tr.solver == rec.solver and tr.batch == 2 and first["sizes"] == [64] * 10
    np.testing.assert_array_equal(first["anchors"], np.asarray(rec.anchors, np.float32))
    assert np.isfinite(np.array(first["losses"])).all()
    stats = np.array(first["region_stats"])
    assert stats.shape == (10, 6) and np.isfinite(stats).all() and (stats[:, 5] > 0).all()
    assert ((stats[:, :5] >= 0) & (stats[:, :5] <= 1)).all()
    assert first["imdb"].augment.jitter == 0.2
    snap = os.path.join(ckpt, "train_iter_10.weights")
    assert DW.read(snap)[3] == 20 and DW.read(snap)[4].size == rec.floats
    # an explicit flag beats the file; a run without --region-stats reports None
    second = pascal_train_yolov2.main(train + ["--iters", "1", "--jitter", "0.1"])
    assert second["imdb"].augment.jitter == 0.1 and second["imdb"].augment.hue == 0.1 and second["region_stats"] is None
    assert "jitter 0.1" in capsys.readouterr().out
    with pytest.raises(SystemExit):                           # the devkit has 20 classes, this cfg 3
        pascal_train_yolov2.main(["--devkit", kit, "--cfg", three, "--dtype", "f32", "--iters", "1"])
    assert "classes=3" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        pascal_train_yolov2.main(train + ["--topology", "paper", "--iters", "1"])
    common = ["--devkit", kit, "--image-set", "trainval", "--batch", "2", "--dtype", "f32"]
    res = pascal_eval_yolov2.main(common + ["--cfg", cfg, "--darknet-weights", snap, "--per-class", "--letterbox"])
    assert res["topology"] == "tiny" and res["detector"].cfg is not None and np.isfinite(res["mAP"])
    assert res["detector"].size == 64                         # --size defaults to the cfg's width
    np.testing.assert_array_equal(res["detector"].anchors, np.asarray(rec.anchors, np.float32))
    with pytest.raises(SystemExit):
        pascal_eval_yolov2.main(common + ["--cfg", three])
    with pytest.raises(SystemExit):
        pascal_eval_yolov2.main(common + ["--cfg", cfg, "--weights", "some.npz"])
    names = tmp_path / "twenty.names"
    names.write_text("".join("thing%d\n" % c for c in range(20)))
    imgs = [os.path.join(golden_dir, "testImg1.jpg"), os.path.join(golden_dir, "testImg2.jpg")]
    detect = ["--cfg", cfg, "--darknet-weights", path, "--size", "160", "--thresh", "0.02", "--dtype", "f32", "--images"] + imgs
    det_file = str(tmp_path / "detections.txt")
    out = pascal_detect_yolov2.main(detect + ["--names", str(names), "--out", det_file])
    assert out["topology"] == "tiny" and len(out["rows"]) > 0 and all(r[1].startswith("thing") for r in out["rows"])
    assert all(line.split()[1].startswith("thing") for line in open(det_file).read().splitlines())
    short = tmp_path / "short.names"
    short.write_text("one\ntwo\n")
    with pytest.raises(SystemExit):
        pascal_detect_yolov2.main(detect + ["--names", str(short)])
    assert "2 names" in capsys.readouterr().err
