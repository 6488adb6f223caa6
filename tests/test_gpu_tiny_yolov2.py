"""GPU tests of the "tiny" topology, the graph of tiny-yolo-voc.cfg: YOLOv2Detector(topology="tiny") filled from a random
tiny `.weights` file against tests/_darknet_tiny_ref.py run end to end in float64 from the same file; the load / save round
trip and the refusal of the other graph's file; the whole backward pass of YOLOv2DarknetTrainer(topology="tiny") against
torch float64 autograd from a fixed random cotangent; the zero padding of the two narrow layers and the last layer's batch
norm under four train steps (f32 and f16, Adam and DarknetSGD with decay) with the snapshot written and reloaded; a resumed
run; and the evaluate, detect and train callers.

Gates: the whole-model one of tests/test_gpu_darknet_yolov2.py (max |d| < 1e-3 max |ref|) and the gradient gates of
tests/test_gpu_darknet_train.py (2e-2 per layer in the Euclidean norm, 1e-4 on moving_var after one step)."""
import os

import numpy as np
import pytest

import _darknet_tiny_ref as T

pytestmark = pytest.mark.gpu

NUM_CLASS, WIDTH_DIV, BATCH = 3, 8, 2
PAD = 16                           # the file's width of layer 0 and of layer 1's input; the stack runs both 32 wide


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


def _detector(size, num_class=NUM_CLASS, dtype="f32", seed=0, topology="tiny"):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    return yolov2.YOLOv2Detector(BATCH, size, num_class=num_class, anchors=yolov2.ANCHORS_TINY_VOC, dtype=dtype,
                                 width_div=WIDTH_DIV, topology=topology, seed=seed)


def _trainer(size, num_class=NUM_CLASS, dtype="f32", seed=0, solver=None):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    return yolov2.YOLOv2DarknetTrainer(BATCH, size, num_class=num_class, anchors=yolov2.ANCHORS_TINY_VOC, dtype=dtype,
                                       width_div=WIDTH_DIV, seed=seed, solver=solver, topology="tiny")


def _write_random_file(tmp_path_factory, num_class, seed, seen):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    file_layers = net_utils._file_layers("tiny", yolov2.yolov2_tiny_specs(num_class, 5, WIDTH_DIV))
    assert len(file_layers) == 9 and file_layers[0][1:3] == (3, PAD) and file_layers[1][1:3] == (PAD, 32)
    assert not file_layers[8][3] and all(l[3] for l in file_layers[:8])
    layers = T.random_layers(file_layers, seed)
    path = str(tmp_path_factory.mktemp("tiny") / ("narrow_tiny_%d.weights" % num_class))
    DW.write(path, layers, seen)
    return path, file_layers, layers


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    """(path, file layer list, the arrays) of a random narrow tiny-yolo-voc file of NUM_CLASS classes, written once"""
    return _write_random_file(tmp_path_factory, NUM_CLASS, 2026, 64000)


@pytest.fixture(scope="module")
def voc_weights_file(tmp_path_factory):
    return _write_random_file(tmp_path_factory, 20, 9, 6)


def _images(size):
    return np.random.default_rng(size).integers(0, 256, (BATCH, size, size, 3), dtype=np.uint8)


def _forward_reference(layers, images_u8):
    return np.stack([T.tiny_forward(layers, (img[:, :, ::-1].astype(np.float64) / 255.0).transpose(2, 0, 1))
                     .transpose(1, 2, 0) for img in images_u8])


# ---------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("size", [64, 96])
def test_tiny_detector_matches_darknet_arithmetic(weights_file, size):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    path, file_layers, _ = weights_file
    det = _detector(size)
    assert det.topology == "tiny" and len(det.networks()) == 2 and det.bn_eps == 1e-6
    assert net_utils.darknet_file_layers(det) == file_layers
    assert net_utils.load_darknet_weights(det, path) == 64000
    x = _images(size)
    grid = host(det.forward(dev(x)))
    S = size // 32
    assert grid.shape == (BATCH, S, S, 5, 5 + NUM_CLASS)
    layers, _used = DW.split(DW.read(path)[4], file_layers)
    ref = _forward_reference(layers, x).reshape(grid.shape)
    err = np.abs(grid - ref).max() / np.abs(ref).max()
    print("tiny topology, f32, size %d: max |d| / max |ref| = %.3e (max |ref| %.3f)" % (size, err, np.abs(ref).max()))
    assert err < 1e-3
    xf = x[..., ::-1].astype(np.float32) / np.float32(255)             # float input is RGB in [0, 1] already
    np.testing.assert_array_equal(host(det.forward(dev(xf))), grid)


# ---------------------------------------------------------------- 2. save and load
def test_save_returns_the_bytes_and_the_other_graph_is_refused(weights_file, tmp_path):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    path, file_layers, layers = weights_file
    det = _detector(64)
    seen = net_utils.load_darknet_weights(det, path)
    p0, p1 = det.stem.export_params()[:2]
    assert p0["W"].shape == (3, 3, 3, 32) and p1["W"].shape == (3, 3, 32, 32)
    np.testing.assert_array_equal(p0["W"][..., :PAD], layers[0]["weights"].transpose(2, 3, 1, 0))
    assert not p0["W"][..., PAD:].any() and not p1["W"][:, :, PAD:, :].any()
    assert not p0["beta"][PAD:].any() and (p0["gamma"][PAD:] == 1).all() and (p0["moving_var"][PAD:] == 1).all()
    back = str(tmp_path / "back.weights")
    net_utils.save_darknet_weights(det, back, seen)
    assert open(back, "rb").read() == open(path, "rb").read()
    assert net_utils.darknet_file_topology(path, NUM_CLASS, 5, WIDTH_DIV) == "tiny"
    # a file of the other Darknet graph, both ways: the float-count error names both
    full = _detector(64, topology="darknet")
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_weights(full, path)
    assert "\"darknet\"" in str(e.value) and "\"tiny\"" in str(e.value) and path in str(e.value)
    other = str(tmp_path / "full.weights")
    DW.write(other, T.random_layers(net_utils.darknet_file_layers(full), 4), 1)
    assert net_utils.darknet_file_topology(other, NUM_CLASS, 5, WIDTH_DIV) == "darknet"
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_weights(det, other)
    assert "\"darknet\"" in str(e.value) and "\"tiny\"" in str(e.value)
    # a non-zero padded entry is not Darknet's function any more: the export refuses it
    params = det.stem.export_params()
    params[1]["W"][0, 0, PAD + 1, 0] = 0.5
    det.stem.load_params(params)
    with pytest.raises(ValueError) as e:
        net_utils.save_darknet_weights(det, str(tmp_path / "no.weights"), 1)
    assert "padded" in str(e.value)
    # a prefix ends at a layer boundary
    DW.write(str(tmp_path / "tiny.conv.6"), layers[:6], 3)
    fresh = _detector(64, seed=3)
    assert net_utils.load_darknet_prefix(fresh, str(tmp_path / "tiny.conv.6")) == 6
    np.testing.assert_array_equal(fresh.stem.export_params()[5]["gamma"], layers[5]["scales"])
    with open(str(tmp_path / "cut.weights"), "wb") as f:
        f.write(open(str(tmp_path / "tiny.conv.6"), "rb").read()[:-8])
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_prefix(fresh, str(tmp_path / "cut.weights"))
    assert "inside layer" in str(e.value)
    with pytest.raises(NotImplementedError) as e:
        yolov2.YOLOv2Trainer(BATCH, 64, num_class=NUM_CLASS, width_div=WIDTH_DIV, topology="tiny")
    assert "YOLOv2DarknetTrainer" in str(e.value)
    for f in (net_utils.save_yolov2_variables, net_utils.restore_yolov2_variables):
        with pytest.raises(ValueError) as e:
            f(fresh, path + ".npz")
        assert "out of scope" in str(e.value)


# ---------------------------------------------------------------- 3. backward
_REFERENCES = {}


def reference(weights_file, size):
    """the float64 training pass from the file at `size`, with the gradients of one fixed cotangent: computed once"""
    if size not in _REFERENCES:
        x = _images(size)
        ref = T.Pass(weights_file[2], x[..., ::-1].astype(np.float64) / 255.0)
        cot = np.random.default_rng(1000 + size).standard_normal(tuple(ref.out.shape)).astype(np.float32)
        _REFERENCES[size] = (x, cot, ref.backward(cot))
    return _REFERENCES[size]


def _real(g, pos):
    """the entries of layer `pos`'s gradient dict that the file holds: the padding of the two narrow layers cut off"""
    if pos == 0:
        return dict(g, W=g["W"][..., :PAD], gamma=g["gamma"][:PAD], beta=g["beta"][:PAD])
    if pos == 1:
        return dict(g, W=g["W"][:, :, :PAD, :])
    return g


@pytest.mark.parametrize("size", [64, 96])
def test_backward_pass_matches_float64_autograd(weights_file, size):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    x, cot, ref = reference(weights_file, size)
    tr = _trainer(size)
    assert tr.topology == "tiny" and len(tr.networks()) == 2 and tr.bn_eps == 1e-6 and tr.cf is None
    assert tr.networks()[1].core_layers == 2
    assert net_utils.load_darknet_weights(tr, weights_file[0]) == 64000
    grid, fine = tr.forward(dev(x), True)
    S = size // 32
    assert tuple(grid.shape) == (BATCH, S, S, 5, 5 + NUM_CLASS)
    out = ref.out.detach().numpy()
    rel = lambda got, want: np.abs(got - want).max() / np.abs(want).max()
    e_grid = rel(host(grid).reshape(out.shape), out)
    tr.backward(dev(cot), fine, size)
    e_cat, e_fine = rel(host(tr.last_dcat), ref.dcat), rel(host(tr.last_dfine), ref.dfine)
    nrm = lambda got, want: np.linalg.norm(got - want) / np.linalg.norm(want)
    errs, pos = {"W": [], "gamma": [], "beta": []}, 0
    for net in tr.networks():
        for full in net.export_grads():
            g = _real(full, pos)
            if pos == 0:            # no gradient reaches the padding: layer 1 reads it through zero filters
                assert not full["W"][..., PAD:].any() and not full["gamma"][PAD:].any() and not full["beta"][PAD:].any()
            if pos == 1:
                assert not full["W"][:, :, PAD:, :].any()
            assert g["W"].shape == ref.dW[pos].shape
            errs["W"].append(nrm(g["W"], ref.dW[pos]))
            if pos < 8:
                errs["gamma"].append(nrm(g["gamma"], ref.dgamma[pos]))
                errs["beta"].append(nrm(g["beta"], ref.dbeta[pos]))
            else:
                e_b = nrm(g["b"], ref.db_last)
            pos += 1
    assert pos == 9
    print("tiny train graph, f32, size %d: grid %.3e, head input %.3e, fine %.3e (max norm); per layer (Euclidean) max dW "
          "%.3e at layer %d, dgamma %.3e, dbeta %.3e, last b %.3e" %
          (size, e_grid, e_cat, e_fine, max(errs["W"]), int(np.argmax(errs["W"])), max(errs["gamma"]), max(errs["beta"]),
           e_b))
    assert e_grid < 1e-3
    for key, es in errs.items():
        for l, e in enumerate(es):
            assert e < 2e-2, (key, l, e)
    assert e_b < 2e-2


def two_objects(size, num_class=NUM_CLASS):
    """a box list (pixels) with two objects per image"""
    truth = np.zeros((BATCH, 30, 5), np.float32)
    u = size / 64.0
    for i in range(BATCH):
        truth[i, 0] = (21.0 * u, 26.0 * u, 23.0 * u, 29.0 * u, i % num_class)
        truth[i, 1] = (44.0 * u, 39.0 * u, 20.0 * u, 18.0 * u, (i + 1) % num_class)
    return dev(truth), dev(np.full(BATCH, 2, np.int32))


def test_moving_variance_after_one_step(weights_file):
    import torch
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    size = 64
    x, _cot, ref = reference(weights_file, size)
    tr = _trainer(size)
    net_utils.load_darknet_weights(tr, weights_file[0])
    before = [p for net in tr.networks() for p in net.export_params()]
    truth, ntruth = two_objects(size)
    tr.step(dev(x), truth=truth, ntruth=ntruth)
    torch.cuda.synchronize()
    after = [p for net in tr.networks() for p in net.export_params()]
    worst = 0.0
    for pos in range(8):
        n = ref.count[pos]
        keep = slice(0, PAD) if pos == 0 else slice(None)
        want = 0.99 * before[pos]["moving_var"][keep].astype(np.float64) + 0.01 * n / (n - 1.0) * ref.batch_var[pos]
        worst = max(worst, float((np.abs(after[pos]["moving_var"][keep] - want) / want).max()))
    print("tiny: moving_var after one step against the float64 reference: max relative error %.3e" % worst)
    assert worst < 1e-4


# ---------------------------------------------------------------- 4. the padded entries under training
def _padded(params):
    """the entries that must not move: the padding of the narrow layers and the last layer's batch norm, as bytes"""
    stem, head = params
    p0, p1, last = stem[0], stem[1], head[-1]
    return {"W0": p0["W"][..., PAD:].tobytes(), "b0": p0["b"][PAD:].tobytes(), "gamma0": p0["gamma"][PAD:].tobytes(),
            "beta0": p0["beta"][PAD:].tobytes(), "mean0": p0["moving_mean"][PAD:].tobytes(),
            "W1": p1["W"][:, :, PAD:, :].tobytes(), "last_gamma": last["gamma"].tobytes(),
            "last_beta": last["beta"].tobytes(), "last_mean": last["moving_mean"].tobytes(),
            "last_var": last["moving_var"].tobytes()}


@pytest.mark.parametrize("solver", ["adam", "sgd"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_padded_entries_stay_put_and_the_snapshot_reloads(weights_file, tmp_path, dtype, solver):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import solver as S
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    size = 64
    sv = S.Solver(burn_in=3, steps=(3,), scales=(0.5,), decay=0.0005) if solver == "sgd" else None
    tr = _trainer(size, dtype=dtype, solver=sv, seed=2)
    assert all(type(o) is (E.DarknetSGD if sv else E.AdamOptimizer) for o in tr.opts) and len(tr.opts) == 2
    fresh = _padded([net.export_params() for net in tr.networks()])      # a fresh model starts in the padded form
    assert not np.frombuffer(fresh["W0"], np.float32).any() and not np.frombuffer(fresh["W1"], np.float32).any()
    assert (np.frombuffer(fresh["gamma0"], np.float32) == 1).all() and not np.frombuffer(fresh["beta0"], np.float32).any()
    net_utils.load_darknet_weights(tr, weights_file[0])
    start = [net.export_params() for net in tr.networks()]
    before = _padded(start)
    assert before["W0"] == fresh["W0"] and before["W1"] == fresh["W1"] and before["gamma0"] == fresh["gamma0"]
    x = dev(_images(size))
    truth, ntruth = two_objects(size)
    for it in range(4):
        loss = tr.step(x, truth=truth, ntruth=ntruth)
        assert np.isfinite(host(loss)).all(), it
    torch.cuda.synchronize()
    end = [net.export_params() for net in tr.networks()]
    after = _padded(end)
    for key in before:
        assert after[key] == before[key], key
    assert not np.array_equal(end[0][0]["W"][..., :PAD], start[0][0]["W"][..., :PAD])        # the real entries train
    assert not np.array_equal(end[0][1]["W"][:, :, :PAD], start[0][1]["W"][:, :, :PAD])
    assert not np.array_equal(end[1][-1]["W"], start[1][-1]["W"]) and not np.array_equal(end[1][-1]["b"], start[1][-1]["b"])
    ckpt = str(tmp_path / "ckpt")
    os.makedirs(ckpt)
    snap = net_utils.save_yolov2_snapshot(tr, ckpt, 4)
    assert snap.endswith("train_iter_4.weights") and net_utils.latest_yolov2_snapshot(ckpt, "tiny") == snap
    det = _detector(size, dtype=dtype, seed=7)
    assert net_utils.restore_yolov2_snapshot(det, snap) == 4
    for a_net, b_net in zip(det.networks(), end):
        for a, b in zip(a_net.export_params(), b_net):
            np.testing.assert_array_equal(a["W"], b["W"])
            np.testing.assert_array_equal(a["beta"], b["beta"])


# ---------------------------------------------------------------- 5. resume
def test_resumed_run_continues_where_the_snapshot_stood(weights_file, tmp_path):
    """2 + 2 steps over a `.weights` snapshot against an uninterrupted 4: the snapshot holds the parameters and moving
    statistics of the uninterrupted run after two steps bit for bit, the resumed trainer stands at its iteration (prior
    term and rate schedule), and the optimizer state starts afresh, as in Darknet -- so the last two steps are finite and
    counted, not bit-equal"""
    import torch
    from tensorflow_yolo2_amd.utils import solver as S
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    size = 64
    sv = S.Solver(burn_in=3, steps=(3,), scales=(0.5,))
    x = dev(_images(size))
    truth, ntruth = two_objects(size)
    whole = _trainer(size, solver=sv)
    net_utils.load_darknet_weights(whole, weights_file[0])
    ckpt = str(tmp_path / "ckpt")
    os.makedirs(ckpt)
    for it in range(4):
        whole.step(x, truth=truth, ntruth=ntruth)
        if it == 1:
            snap = net_utils.save_yolov2_snapshot(whole, ckpt, 2)
            at_two = [net.export_params() for net in whole.networks()]
    torch.cuda.synchronize()
    resumed = _trainer(size, solver=sv, seed=11)
    assert net_utils.restore_yolov2_snapshot(resumed, net_utils.latest_yolov2_snapshot(ckpt, "tiny")) == 2
    assert resumed.iteration == 2 and all(o.t == 2 for o in resumed.opts)
    for a_net, b_net in zip(resumed.networks(), at_two):
        for l, (a, b) in enumerate(zip(a_net.export_params(), b_net)):
            for k in ("W", "gamma", "beta", "moving_var"):
                if (a_net is resumed.networks()[0] and l == 0 and k == "moving_var"):
                    continue                     # the padded filters' moving variance is not in the file: it restarts at 1
                assert a[k].tobytes() == b[k].tobytes(), (l, k)
    for _ in range(2):
        loss = resumed.step(x, truth=truth, ntruth=ntruth)
        assert np.isfinite(host(loss)).all()
    assert resumed.iteration == whole.iteration == 4
    a = net_utils.save_yolov2_snapshot(resumed, str(tmp_path), 4)
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    assert DW.read(a)[3] == 4 * BATCH


# ---------------------------------------------------------------- 6. the callers
def test_callers_take_a_tiny_file(voc_weights_file, tmp_path, golden_dir):
    from test_box_list_host import build_devkit
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2, pascal_eval_yolov2, pascal_train_yolov2
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    path, _file_layers, layers = voc_weights_file
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    ckpt = str(tmp_path / "ckpt")
    common = ["--devkit", kit, "--width-div", "8", "--batch", "2", "--size", "64", "--dtype", "f32"]
    first = pascal_train_yolov2.main(common + ["--darknet-weights", path, "--iters", "1", "--ckpt-dir", ckpt])
    assert first["topology"] == "tiny" and isinstance(first["trainer"], yolov2.YOLOv2DarknetTrainer)
    assert first["trainer"].topology == "tiny" and np.isfinite(np.array(first["losses"])).all()
    np.testing.assert_array_equal(first["anchors"], np.asarray(yolov2.ANCHORS_TINY_VOC, np.float32))
    snap1 = os.path.join(ckpt, "train_iter_1.weights")
    assert DW.read(snap1)[3] == 2
    second = pascal_train_yolov2.main(common + ["--topology", "tiny", "--ckpt-dir", ckpt, "--iters", "1", "--box-labels",
                                               "--solver", "darknet", "--burn-in", "3"])
    assert (second["first_iter"], second["last_iter"]) == (2, 2) and second["trainer"].iteration == 2
    snap2 = os.path.join(ckpt, "train_iter_2.weights")
    assert DW.read(snap2)[3] == 4
    # a directory of the other Darknet graph's snapshots fails in the loader, by the float count
    with pytest.raises(ValueError) as e:
        pascal_train_yolov2.main(common + ["--topology", "darknet", "--ckpt-dir", ckpt, "--iters", "1"])
    assert "floats" in str(e.value) and "\"tiny\"" in str(e.value)
    with pytest.raises(SystemExit):
        pascal_train_yolov2.main(common + ["--topology", "darknet", "--darknet-weights", path, "--iters", "1"])
    core = str(tmp_path / "tiny.conv.6")
    DW.write(core, layers[:6], 9)
    third = pascal_train_yolov2.main(common + ["--topology", "tiny", "--darknet-backbone", core, "--iters", "1"])
    assert third["topology"] == "tiny" and np.isfinite(np.array(third["losses"])).all()
    res = pascal_eval_yolov2.main(common + ["--image-set", "trainval", "--per-class", "--letterbox",
                                            "--darknet-weights", snap2])
    assert res["topology"] == "tiny" and len(res["detector"].networks()) == 2 and np.isfinite(res["mAP"])
    np.testing.assert_array_equal(res["detector"].anchors, np.asarray(yolov2.ANCHORS_TINY_VOC, np.float32))
    res = pascal_eval_yolov2.main(common + ["--image-set", "trainval", "--protocol", "darknet", "--darknet-weights", snap2])
    assert res["topology"] == "tiny" and np.isfinite(res["mAP"])
    images = [os.path.join(golden_dir, "testImg1.jpg"), os.path.join(golden_dir, "testImg2.jpg")]
    for extra in ([], ["--stretch"], ["--protocol", "darknet"]):
        out = pascal_detect_yolov2.main(["--darknet-weights", path, "--images"] + images +
                                        ["--width-div", "8", "--size", "160", "--thresh", "0.02", "--dtype", "f32"] + extra)
        assert out["topology"] == "tiny" and out["detector"].topology == "tiny" and len(out["rows"]) > 0
        assert all(np.isfinite(r[2]) for r in out["rows"])
