"""GPU tests of the Darknet import: y2_passthrough_concat_darknet and y2_u8_bgr_to_f32_rgb against their numpy
specifications (bit for bit), YOLOv2Detector(topology="darknet") filled from a `.weights` file against
tests/_darknet_ref.py run end to end in float64 from the same file, the load / save round trip, the detect and evaluation
callers with --darknet-weights, and the Darknet-19 backbone of such a file in the paper-topology trainer, by hand and
through pascal_train_yolov2 --darknet-backbone with its snapshot and resume.

The whole-model gate is the one the composed f32 detector is held to (tests/test_ext.py): max |d| < 1e-3 max |ref|."""
import ctypes as C
import os

import numpy as np
import pytest

import _darknet_ref as D

pytestmark = pytest.mark.gpu

NUM_CLASS, WIDTH_DIV, BATCH = 3, 8, 2
Y2_OK, Y2_ERR_ARG = 0, -1          # include/yolo2_hip.h


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- 5. the two kernels
@pytest.mark.parametrize("shape", [(2, 3, 3, 64, 32), (2, 2, 3, 8, 4), (1, 1, 1, 4, 1), (3, 13, 13, 64, 1024)])
def test_passthrough_concat_darknet_is_the_specification(shape):
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import darknet_reorg as RG
    n, h, w, cf, cc = shape
    rng = np.random.default_rng(sum(shape))
    fine = rng.standard_normal((n, 2 * h, 2 * w, cf)).astype(np.float32)
    coarse = rng.standard_normal((n, h, w, cc)).astype(np.float32)
    out = E.passthrough_concat_darknet(dev(fine), dev(coarse))
    assert tuple(out.shape) == (n, h, w, 4 * cf + cc)
    np.testing.assert_array_equal(out.cpu().numpy(), RG.passthrough_concat_darknet(fine, coarse))


def test_passthrough_concat_darknet_refuses_bad_arguments():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    fine = torch.zeros(2 * 2 * 2 * 8, device="cuda")
    coarse = torch.zeros(4, device="cuda")
    out = torch.zeros(36, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    call = lambda f, c, o, *dims: lib.y2_passthrough_concat_darknet(f, c, o, *dims, null)
    assert call(p(fine), p(coarse), p(out), 1, 1, 1, 8, 4) == Y2_OK
    for args in ((null, p(coarse), p(out), 1, 1, 1, 8, 4), (p(fine), null, p(out), 1, 1, 1, 8, 4),
                 (p(fine), p(coarse), null, 1, 1, 1, 8, 4),
                 (p(fine), p(coarse), p(out), 1, 1, 1, 6, 4), (p(fine), p(coarse), p(out), 1, 1, 1, 2, 4),
                 (p(fine), p(coarse), p(out), 0, 1, 1, 8, 4), (p(fine), p(coarse), p(out), 1, 0, 1, 8, 4),
                 (p(fine), p(coarse), p(out), 1, 1, -1, 8, 4), (p(fine), p(coarse), p(out), 1, 1, 1, 0, 4),
                 (p(fine), p(coarse), p(out), 1, 1, 1, 8, 0)):
        assert call(*args) == Y2_ERR_ARG, args[3:]
        assert b"y2_passthrough_concat_darknet" in lib.y2_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", [(1, 1, 3), (2, 64, 64, 3), (7, 9, 3)])
def test_u8_to_darknet_input_is_the_numpy_quotient(shape):
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(len(shape) + shape[0])
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    if x.size >= 768:
        x.reshape(-1)[:768] = np.repeat(np.arange(256, dtype=np.uint8), 3)          # every byte value, in every channel
    ref = x[..., ::-1].astype(np.float32) / np.float32(255)
    got = E.u8_to_darknet_input(dev(x))
    assert got.dtype.is_floating_point and tuple(got.shape) == shape
    np.testing.assert_array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------- 6. the whole model
def _detector(size, num_class=NUM_CLASS, dtype="f32", seed=0):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    return yolov2.YOLOv2Detector(BATCH, size, num_class=num_class, dtype=dtype, width_div=WIDTH_DIV, topology="darknet",
                                 seed=seed)


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    """(path, file layer list, the arrays) of a random narrow yolov2-voc file of NUM_CLASS classes, written once"""
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    file_layers = net_utils.darknet_file_layers(_detector(64))
    assert len(file_layers) == 23 and file_layers[3][0] == 1 and not file_layers[22][3]
    layers = D.random_layers(file_layers, 2024)
    path = str(tmp_path_factory.mktemp("darknet") / "narrow.weights")
    DW.write(path, layers, 64000)
    return path, file_layers, layers


def _reference(path, file_layers, images_u8):
    """tests/_darknet_ref.py end to end from the file -> [N][S][S][B * (5 + C)] float64"""
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    layers, used = DW.split(DW.read(path)[4], file_layers)
    assert len(layers) == 23
    out = []
    for img in images_u8:
        x = (img[:, :, ::-1].astype(np.float64) / 255.0).transpose(2, 0, 1)
        out.append(D.yolov2_voc_forward(layers, x).transpose(1, 2, 0))
    return np.stack(out)


@pytest.mark.parametrize("size", [64, 96])
def test_darknet_detector_matches_darknet_arithmetic(weights_file, size):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    path, file_layers, _ = weights_file
    det = _detector(size)
    assert len(det.networks()) == 4 and det.bn_eps == 1e-6
    assert net_utils.load_darknet_weights(det, path) == 64000
    rng = np.random.default_rng(size)
    x = rng.integers(0, 256, (BATCH, size, size, 3), dtype=np.uint8)
    grid = det.forward(dev(x)).cpu().numpy()
    S = size // 32
    assert grid.shape == (BATCH, S, S, 5, 5 + NUM_CLASS)
    ref = _reference(path, file_layers, x).reshape(grid.shape)
    err = np.abs(grid - ref).max() / np.abs(ref).max()
    print("darknet topology, f32, size %d: max |d| / max |ref| = %.3e (max |ref| %.3f)" % (size, err, np.abs(ref).max()))
    assert err < 1e-3
    # float input is RGB in [0, 1] already
    xf = x[..., ::-1].astype(np.float32) / np.float32(255)
    np.testing.assert_array_equal(det.forward(dev(xf)).cpu().numpy(), grid)


def test_load_refuses_a_file_of_another_model(weights_file):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    path, _, _ = weights_file
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_weights(_detector(64, num_class=4), path)
    assert "4 classes" in str(e.value) and path in str(e.value)
    with pytest.raises(ValueError):
        net_utils.load_darknet_weights(yolov2.YOLOv2Detector(BATCH, 64, num_class=NUM_CLASS, dtype="f32",
                                                             width_div=WIDTH_DIV), path)
    det = _detector(64)
    for f in (net_utils.save_yolov2_variables, net_utils.restore_yolov2_variables):
        with pytest.raises(ValueError) as e:
            f(det, path + ".npz")
        assert "out of scope" in str(e.value)
    with pytest.raises(NotImplementedError):
        yolov2.YOLOv2Trainer(BATCH, 64, num_class=NUM_CLASS, width_div=WIDTH_DIV, topology="darknet")


# ---------------------------------------------------------------- 7. round trip
def test_save_returns_the_bytes_and_folds_a_bias(weights_file, tmp_path):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    path, _, _ = weights_file
    det = _detector(64)
    seen = net_utils.load_darknet_weights(det, path)
    back = str(tmp_path / "back.weights")
    net_utils.save_darknet_weights(det, back, seen)
    assert open(back, "rb").read() == open(path, "rb").read()
    # conv biases everywhere, and a last layer whose batch norm is no identity: the export folds both
    rng = np.random.default_rng(5)
    for net in det.networks():
        params = net.export_params()
        for p in params:
            p["b"] = rng.normal(0, 0.3, p["b"].shape).astype(np.float32)
        if net is det.head:
            n = params[-1]["b"].size
            params[-1].update(gamma=rng.uniform(0.7, 1.3, n).astype(np.float32), beta=rng.normal(0, 0.2, n).astype(np.float32),
                              moving_mean=rng.normal(0, 0.2, n).astype(np.float32),
                              moving_var=rng.uniform(0.5, 2.0, n).astype(np.float32))
        net.load_params(params)
    x = dev(rng.integers(0, 256, (BATCH, 64, 64, 3), dtype=np.uint8))
    want = det.forward(x).cpu().numpy().copy()
    folded = str(tmp_path / "folded.weights")
    net_utils.save_darknet_weights(det, folded, 1)
    other = _detector(64, seed=9)
    assert net_utils.load_darknet_weights(other, folded) == 1
    got = other.forward(x).cpu().numpy()
    assert np.abs(got - want).max() < 1e-3 * np.abs(want).max()
    assert not np.array_equal(other.head.export_params()[-1]["b"], det.head.export_params()[-1]["b"])
    det.head.set_layer_options(slopes=[0.1, 0.1])
    with pytest.raises(ValueError) as e:
        net_utils.save_darknet_weights(det, str(tmp_path / "no.weights"), 1)
    assert "slope" in str(e.value)


# ---------------------------------------------------------------- 8. the detect caller
@pytest.fixture(scope="module")
def voc_weights_file(tmp_path_factory):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    file_layers = net_utils.darknet_file_layers(_detector(64, num_class=20))
    path = str(tmp_path_factory.mktemp("darknet_voc") / "narrow_voc.weights")
    DW.write(path, D.random_layers(file_layers, 7), 5)
    return path


@pytest.mark.parametrize("stretch", [False, True])
def test_detect_caller_runs_a_darknet_file(voc_weights_file, golden_dir, stretch):
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2 as det_main
    images = [os.path.join(golden_dir, "testImg1.jpg"), os.path.join(golden_dir, "testImg2.jpg")]
    argv = ["--darknet-weights", voc_weights_file, "--images"] + images + \
           ["--width-div", "8", "--size", "160", "--thresh", "0.02", "--keep-grids"]
    res = det_main.main(argv + ["--dtype", "f32"] + (["--stretch"] if stretch else []))
    detector, pool = res["detector"], res["pool"]
    assert detector.topology == "darknet" and len(detector.networks()) == 4
    batch, valid = pool.batch(160, 0, letterbox=not stretch, fill=127)
    det, score, count = detector.detect_batch(batch, pool.table, pool.eval_index, 0.02, 0.45, 100, letterbox=not stretch)
    det, score, count = det.cpu().numpy(), score.cpu().numpy(), count.cpu().numpy()
    rows = [(pool.paths[k], int(d[4]), float(s), int(d[0]), int(d[1]), int(d[2]), int(d[3]))
            for k in range(valid) for d, s in zip(det[k, :count[k]], score[k, :count[k]])]
    assert len(rows) > 0 and valid == 2
    from tensorflow_yolo2_amd.img_dataset import pascal_voc
    assert [(r[0], pascal_voc.CLASSES.index(r[1])) + r[2:] for r in res["rows"]] == rows
    # the same run in f16: it completes with finite scores; its head against the f32 one is reported, not gated
    half = det_main.main(argv + ["--dtype", "f16"] + (["--stretch"] if stretch else []))
    assert all(np.isfinite(r[2]) for r in half["rows"])
    g16, g32 = half["grids"].cpu().numpy(), res["grids"].cpu().numpy()
    assert np.isfinite(g16).all()
    print("darknet topology, f16 against f32 head (%s): max |d| / max |ref| = %.3e" %
          ("stretch" if stretch else "letterbox", np.abs(g16 - g32).max() / np.abs(g32).max()))
    with pytest.raises(SystemExit):
        det_main.parse_args(["--darknet-weights", voc_weights_file, "--weights", "x.npz", "--images"] + images)


# ---------------------------------------------------------------- 9. the backbone in the paper-topology trainer
def test_darknet_backbone_in_the_trainer_and_its_snapshot(weights_file, tmp_path):
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.utils import yolov2_snapshot as V2
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    _, file_layers, layers = weights_file
    core = str(tmp_path / "narrow.conv.18")
    DW.write(core, layers[:18], 9)                                   # ends at a layer boundary, as darknet19_448.conv.23
    with pytest.raises(ValueError) as e:
        net_utils.read_darknet_backbone(core, 1e-3, width_div=WIDTH_DIV)
    assert "YOLOv2Trainer(bn_eps=1e-6)" in str(e.value)
    mk = lambda **kw: yolov2.YOLOv2Trainer(BATCH, 64, num_class=20, dtype="f32", width_div=WIDTH_DIV, **kw)
    trainer = mk(bn_eps=1e-6)
    stem, deep, head = trainer.networks()
    assert stem.bn_eps == deep.bn_eps == head.bn_eps == 1e-6
    dicts = net_utils.read_darknet_backbone(core, trainer.bn_eps, width_div=WIDTH_DIV)
    assert len(dicts) == 18 and net_utils.load_darknet19_backbone(trainer, dicts) == 18
    sp, dp = stem.export_params(), deep.export_params()
    w0 = layers[0]["weights"].transpose(2, 3, 1, 0)
    np.testing.assert_array_equal(sp[0]["W"], w0[:, :, ::-1, :] * np.float32(0.5))
    k0 = 0.5 * layers[0]["weights"].astype(np.float64).sum(axis=(1, 2, 3))
    np.testing.assert_allclose(sp[0]["moving_mean"], layers[0]["rolling_mean"] - k0, rtol=0, atol=1e-6)
    assert sp[3]["W"].shape[0] == 3                                  # Darknet's 1x1 fourth layer on the centre tap
    np.testing.assert_array_equal(sp[3]["W"][1, 1], layers[3]["weights"][:, :, 0, 0].T)
    off = sp[3]["W"].copy()
    off[1, 1] = 0
    assert not off.any()
    np.testing.assert_array_equal(sp[12]["gamma"], layers[12]["scales"])
    np.testing.assert_array_equal(dp[4]["W"], layers[17]["weights"].transpose(2, 3, 1, 0))
    np.testing.assert_array_equal(dp[4]["moving_var"], layers[17]["rolling_variance"])
    np.testing.assert_array_equal(dp[4]["beta"], layers[17]["biases"])
    assert not dp[4]["b"].any()
    rng = np.random.default_rng(3)
    images = dev(rng.integers(0, 256, (BATCH, 64, 64, 3), dtype=np.uint8))
    labels = dev(synthetic.det_labels(BATCH, 64, 2, 11))
    loss = trainer.step(images, labels)
    torch.cuda.synchronize()
    assert np.isfinite(loss.cpu().numpy()).all()
    snap = str(tmp_path / "eps.npz")
    net_utils.save_yolov2_variables(trainer, snap)
    with np.load(snap) as z:
        assert float(z["yolov2/bn_eps"]) == 1e-6
    assert net_utils.read_yolov2_bn_eps(snap) == 1e-6
    plain = mk()
    with pytest.raises(ValueError) as e:
        net_utils.restore_yolov2_variables(plain, snap)
    assert "1e-06" in str(e.value) and "0.001" in str(e.value)
    assert net_utils.restore_yolov2_variables(mk(bn_eps=1e-6), snap) == 1
    # a default trainer's snapshot has the key set it had before
    snap0 = str(tmp_path / "plain.npz")
    keys = net_utils.save_yolov2_variables(plain, snap0)
    assert "yolov2/bn_eps" not in keys and net_utils.read_yolov2_bn_eps(snap0) is None
    st = {s: net.export_params() for s, net in zip(V2.STACKS, plain.networks())}
    before = V2.to_blob(st, plain.anchors, 20, 0, adam={s: {"m": [{k: d[k] for k in V2.PARAM_KEYS} for d in st[s]],
                                                          "v": [{k: d[k] for k in V2.PARAM_KEYS} for d in st[s]], "t": 0}
                                                      for s in V2.STACKS})
    assert sorted(k for k in keys if not k.startswith("yolov2/scaler/")) == sorted(before)


# ---------------------------------------------------------------- the train and evaluation callers
def test_train_and_eval_callers_take_darknet_files(weights_file, voc_weights_file, tmp_path, golden_dir):
    from test_box_list_host import build_devkit
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2, pascal_train_yolov2
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    core, ckpt = str(tmp_path / "narrow.conv.18"), str(tmp_path / "ckpt")
    DW.write(core, weights_file[2][:18], 9)
    common = ["--devkit", kit, "--width-div", "8", "--batch", "2", "--size", "64", "--dtype", "f32"]
    first = pascal_train_yolov2.main(common + ["--ckpt-dir", ckpt, "--iters", "1", "--darknet-backbone", core])
    assert first["trainer"].bn_eps == 1e-6 and np.isfinite(np.array(first["losses"])).all()
    with np.load(os.path.join(ckpt, "train_iter_1.npz")) as z:
        assert float(z["yolov2/bn_eps"]) == 1e-6
    second = pascal_train_yolov2.main(common + ["--ckpt-dir", ckpt, "--iters", "1"])      # the epsilon is the snapshot's
    assert second["trainer"].bn_eps == 1e-6 and (second["first_iter"], second["last_iter"]) == (2, 2)
    ev = ["--image-set", "trainval", "--per-class", "--letterbox"]
    res = pascal_eval_yolov2.main(common + ev + ["--ckpt-dir", ckpt])
    assert res["detector"].bn_eps == 1e-6 and res["detector"].topology == "paper" and res["restored"] == 2
    res = pascal_eval_yolov2.main(common + ev + ["--darknet-weights", voc_weights_file])
    assert res["detector"].topology == "darknet" and len(res["detector"].networks()) == 4 and np.isfinite(res["mAP"])
    with pytest.raises(SystemExit):
        pascal_eval_yolov2.parse_args(common + ["--darknet-weights", voc_weights_file, "--ckpt-dir", ckpt])
    with pytest.raises(SystemExit):
        pascal_train_yolov2.parse_args(common + ["--darknet-backbone", core, "--imagenet-ckpt-dir", ckpt])
