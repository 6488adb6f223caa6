"""GPU tests of training the yolov2-voc.cfg graph: y2_passthrough_concat_darknet_backward against its numpy
specification (bit for bit), the whole backward pass of YOLOv2DarknetTrainer against torch float64 autograd of Darknet's
arithmetic (tests/_darknet_train_ref.py) from a fixed random cotangent, the gradient masks and the moving statistics,
whole train steps in f32 and f16, the file round trip (train, save, load into a detector) and the train caller.

The gradient gates are the ones tests/test_ext.py holds the paper graph to: grid 1e-3, concat 2e-3, fine 5e-3 (max
norm, relative to the reference's maximum), 2e-2 per layer in the Euclidean norm."""
import ctypes as C
import os

import numpy as np
import pytest

import _darknet_ref as D
import _darknet_train_ref as TR

pytestmark = pytest.mark.gpu

NUM_CLASS, WIDTH_DIV, BATCH = 3, 8, 2
Y2_OK, Y2_ERR_ARG = 0, -1          # include/yolo2_hip.h


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy().copy()


# ---------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("shape", [(1, 1, 1, 4, 1), (2, 2, 3, 8, 4), (2, 3, 2, 8, 3), (2, 3, 3, 64, 32),
                                   (3, 13, 13, 64, 1024)])
def test_passthrough_concat_darknet_backward_is_the_specification(shape):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import darknet_reorg as RG
    n, h, w, cf, cc = shape
    rng = np.random.default_rng(sum(shape))
    dout = rng.standard_normal((n, h, w, 4 * cf + cc)).astype(np.float32)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    dfine, dcoarse = nan(n, 2 * h, 2 * w, cf), nan(n, h, w, cc)
    got = E.passthrough_concat_darknet_backward(dev(dout), cf, dfine_out=dfine, dcoarse_out=dcoarse)
    assert got[0] is dfine and got[1] is dcoarse
    want_fine, want_coarse = RG.passthrough_concat_darknet_backward(dout, cf)
    np.testing.assert_array_equal(host(dfine).view(np.uint32), want_fine.view(np.uint32))
    np.testing.assert_array_equal(host(dcoarse).view(np.uint32), want_coarse.view(np.uint32))
    # the gradient of a permutation beside a copy is its inverse: forward, then backward, returns the inputs
    fine = rng.standard_normal((n, 2 * h, 2 * w, cf)).astype(np.float32)
    coarse = rng.standard_normal((n, h, w, cc)).astype(np.float32)
    f2, c2 = E.passthrough_concat_darknet_backward(E.passthrough_concat_darknet(dev(fine), dev(coarse)), cf)
    assert tuple(f2.shape) == fine.shape and tuple(c2.shape) == coarse.shape
    np.testing.assert_array_equal(host(f2).view(np.uint32), fine.view(np.uint32))
    np.testing.assert_array_equal(host(c2).view(np.uint32), coarse.view(np.uint32))


def test_passthrough_concat_darknet_backward_refuses_bad_arguments():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    dout = torch.zeros(36, device="cuda")
    dfine = torch.zeros(2 * 2 * 8, device="cuda")
    dcoarse = torch.zeros(4, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    call = lambda o, f, c, *dims: lib.y2_passthrough_concat_darknet_backward(o, f, c, *dims, null)
    assert call(p(dout), p(dfine), p(dcoarse), 1, 1, 1, 8, 4) == Y2_OK
    for args in ((null, p(dfine), p(dcoarse), 1, 1, 1, 8, 4), (p(dout), null, p(dcoarse), 1, 1, 1, 8, 4),
                 (p(dout), p(dfine), null, 1, 1, 1, 8, 4),
                 (p(dout), p(dfine), p(dcoarse), 1, 1, 1, 6, 4), (p(dout), p(dfine), p(dcoarse), 1, 1, 1, 2, 4),
                 (p(dout), p(dfine), p(dcoarse), 0, 1, 1, 8, 4), (p(dout), p(dfine), p(dcoarse), 1, 0, 1, 8, 4),
                 (p(dout), p(dfine), p(dcoarse), 1, 1, -1, 8, 4), (p(dout), p(dfine), p(dcoarse), 1, 1, 1, 0, 4),
                 (p(dout), p(dfine), p(dcoarse), 1, 1, 1, 8, 0),
                 (p(dout), p(dfine), p(dcoarse), 1, 8192, 8192, 8, 4)):        # 16 H W Cf beyond 32-bit indices
        assert call(*args) == Y2_ERR_ARG, args[3:]
        assert b"y2_passthrough_concat_darknet_backward" in lib.y2_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the model, its file and its reference
def _trainer(size, num_class=NUM_CLASS, dtype="f32", seed=0, solver=None):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    return yolov2.YOLOv2DarknetTrainer(BATCH, size, num_class=num_class, dtype=dtype, width_div=WIDTH_DIV, seed=seed,
                                       solver=solver)


def _detector(size, num_class=NUM_CLASS, dtype="f32", seed=0):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    return yolov2.YOLOv2Detector(BATCH, size, num_class=num_class, dtype=dtype, width_div=WIDTH_DIV, topology="darknet",
                                 seed=seed)


def _write_random_file(tmp_path_factory, num_class, seed, seen):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    file_layers = net_utils.darknet_file_layers(_trainer(64, num_class=num_class))
    assert len(file_layers) == 23 and file_layers[3][0] == 1 and not file_layers[22][3]
    layers = D.random_layers(file_layers, seed)
    path = str(tmp_path_factory.mktemp("darknet_train") / ("narrow_%d.weights" % num_class))
    DW.write(path, layers, seen)
    return path, file_layers, layers


@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    """(path, file layer list, the arrays) of a random narrow yolov2-voc file of NUM_CLASS classes, written once"""
    return _write_random_file(tmp_path_factory, NUM_CLASS, 2025, 64000)


@pytest.fixture(scope="module")
def voc_weights_file(tmp_path_factory):
    return _write_random_file(tmp_path_factory, 20, 8, 6)


def _images(size):
    return np.random.default_rng(size).integers(0, 256, (BATCH, size, size, 3), dtype=np.uint8)


_REFERENCES = {}


def reference(weights_file, size):
    """the float64 training pass from the file at `size`, with the gradients of one fixed cotangent: computed once"""
    if size not in _REFERENCES:
        x = _images(size)
        ref = TR.Pass(weights_file[2], x[..., ::-1].astype(np.float64) / 255.0)
        cot = np.random.default_rng(1000 + size).standard_normal(tuple(ref.out.shape)).astype(np.float32)
        _REFERENCES[size] = (x, cot, ref.backward(cot))
    return _REFERENCES[size]


def two_objects(size, num_class=NUM_CLASS):
    """a box list (pixels) with two objects per image"""
    truth = np.zeros((BATCH, 30, 5), np.float32)
    u = size / 64.0
    for i in range(BATCH):
        truth[i, 0] = (21.0 * u, 26.0 * u, 23.0 * u, 29.0 * u, i % num_class)
        truth[i, 1] = (44.0 * u, 39.0 * u, 20.0 * u, 18.0 * u, (i + 1) % num_class)
    return dev(truth), dev(np.full(BATCH, 2, np.int32))


# ---------------------------------------------------------------- 2. whole-step gradients
@pytest.mark.parametrize("size", [64, 96])
def test_backward_pass_matches_float64_autograd(weights_file, size):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    x, cot, ref = reference(weights_file, size)
    tr = _trainer(size)
    assert tr.topology == "darknet" and len(tr.networks()) == 4 and tr.bn_eps == 1e-6
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
        for g in net.export_grads():
            assert g["W"].shape == ref.dW[pos].shape
            errs["W"].append(nrm(g["W"], ref.dW[pos]))
            if pos < 22:
                errs["gamma"].append(nrm(g["gamma"], ref.dgamma[pos]))
                errs["beta"].append(nrm(g["beta"], ref.dbeta[pos]))
            else:
                e_b = nrm(g["b"], ref.db_last)
            pos += 1
    assert pos == 23
    print("darknet train graph, f32, size %d: grid %.3e, dcat %.3e, dfine %.3e (max norm); per layer (Euclidean) max dW "
          "%.3e at layer %d, dgamma %.3e, dbeta %.3e, last b %.3e" %
          (size, e_grid, e_cat, e_fine, max(errs["W"]), int(np.argmax(errs["W"])), max(errs["gamma"]), max(errs["beta"]),
           e_b))
    assert e_grid < 1e-3
    assert e_cat < 2e-3
    assert e_fine < 5e-3
    for key, es in errs.items():
        for l, e in enumerate(es):
            assert e < 2e-2, (key, l, e)
    assert e_b < 2e-2


# ---------------------------------------------------------------- 3. masks and moving statistics
def _off_centre(W):
    W = W.copy()
    W[1, 1] = 0
    return W


@pytest.mark.parametrize("solver", ["adam", "sgd"])
def test_masks_hold_and_moving_statistics_move(weights_file, solver):
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import solver as S
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    size = 64
    x, _cot, ref = reference(weights_file, size)
    sv = S.Solver(burn_in=3, steps=(3,), scales=(0.5,)) if solver == "sgd" else None
    tr = _trainer(size, solver=sv)
    assert all(type(o) is (E.DarknetSGD if sv else E.AdamOptimizer) for o in tr.opts) and len(tr.opts) == 4
    net_utils.load_darknet_weights(tr, weights_file[0])
    before = [net.export_params() for net in tr.networks()]
    assert not _off_centre(before[0][3]["W"]).any() and before[0][3]["W"][1, 1].any()
    truth, ntruth = two_objects(size)
    worst = 0.0
    for it in range(3):
        loss = tr.step(dev(x), truth=truth, ntruth=ntruth)
        torch.cuda.synchronize()
        assert np.isfinite(host(loss)).all()
        after = [net.export_params() for net in tr.networks()]
        assert not _off_centre(after[0][3]["W"]).any(), it
        if it == 0:
            # Darknet's rolling_variance: .99 old + .01 n / (n - 1) of the batch variance
            pos = 0
            for b_net, a_net in zip(before, after):
                for b, a in zip(b_net, a_net):
                    if pos < 22:
                        n = ref.count[pos]
                        want = 0.99 * b["moving_var"].astype(np.float64) + 0.01 * n / (n - 1.0) * ref.batch_var[pos]
                        worst = max(worst, float((np.abs(a["moving_var"] - want) / want).max()))
                    pos += 1
            print("moving_var after one step against the float64 reference (%s): max relative error %.3e" % (solver, worst))
            assert worst < 1e-4
    last_b, last_a = before[3][-1], after[3][-1]
    for k in ("gamma", "beta", "moving_mean", "moving_var"):
        assert last_a[k].tobytes() == last_b[k].tobytes(), k
    assert np.array_equal(last_a["gamma"], np.full(last_a["gamma"].shape, np.sqrt(1.0 + 1e-6), np.float32))
    assert not np.array_equal(last_a["W"], last_b["W"]) and not np.array_equal(last_a["b"], last_b["b"])
    assert not np.array_equal(after[0][3]["W"][1, 1], before[0][3]["W"][1, 1])
    pos = 0
    for b_net, a_net in zip(before, after):
        for b, a in zip(b_net, a_net):
            if pos < 22:
                assert not np.array_equal(a["moving_mean"], b["moving_mean"]), pos
                assert not np.array_equal(a["moving_var"], b["moving_var"]), pos
            pos += 1


# ---------------------------------------------------------------- 4. training behaves
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_eight_steps_lower_the_loss(weights_file, dtype):
    import torch
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    size = 96
    tr = _trainer(size, dtype=dtype)
    net_utils.load_darknet_weights(tr, weights_file[0])
    x = dev(_images(size))
    truth, ntruth = two_objects(size)
    losses = [float(tr.step(x, truth=truth, ntruth=ntruth)[4]) for _ in range(8)]
    print("darknet trainer, %s, eight steps on one batch: total loss %s" % (dtype, ["%.4f" % v for v in losses]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    truth2, ntruth2 = two_objects(128)
    l2 = tr.step(dev(_images(128)), truth=truth2, ntruth=ntruth2)
    assert np.isfinite(float(l2[4])) and len(tr.ctx) == 2 and tr.iteration == 9
    for a, b in zip(tr.ctx[128], tr.ctx[size]):
        assert a.params.data_ptr() == b.params.data_ptr() and a.state.data_ptr() == b.state.data_ptr()
    for net in tr.networks():
        assert torch.isfinite(net.params).all() and torch.isfinite(net.state).all()
    # the masks hold in the loss-scaled mode and across sizes too
    assert not _off_centre(tr.networks()[0].export_params()[3]["W"]).any()
    last = tr.networks()[3].export_params()[-1]
    assert np.array_equal(last["moving_var"], np.ones_like(last["moving_var"])) and not last["beta"].any()
    assert not last["moving_mean"].any()


# ---------------------------------------------------------------- 5. the loop closes
def test_trained_model_is_written_and_read_back(weights_file, tmp_path):
    import torch
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    path, file_layers, layers = weights_file
    size = 64
    tr = _trainer(size)
    net_utils.load_darknet_weights(tr, path)
    x = _images(size)
    truth, ntruth = two_objects(size)
    for _ in range(2):
        tr.step(dev(x), truth=truth, ntruth=ntruth)
    torch.cuda.synchronize()
    out = str(tmp_path / "trained.weights")
    net_utils.save_darknet_weights(tr, out, 64000 + 2 * BATCH)
    assert DW.read(out)[3] == 64000 + 2 * BATCH
    assert open(out, "rb").read() != open(path, "rb").read()
    det = _detector(size, seed=5)
    assert net_utils.load_darknet_weights(det, out) == 64000 + 2 * BATCH
    grid = host(det.forward(dev(x)))
    written, _used = DW.split(DW.read(out)[4], file_layers)
    assert len(written) == 23
    ref = np.stack([D.yolov2_voc_forward(written, (img[:, :, ::-1].astype(np.float64) / 255.0).transpose(2, 0, 1))
                    .transpose(1, 2, 0) for img in x]).reshape(grid.shape)
    err = np.abs(grid - ref).max() / np.abs(ref).max()
    print("trained and written model in a fresh detector against Darknet's arithmetic: max |d| / max |ref| = %.3e" % err)
    assert err < 1e-3
    # a fresh (never loaded) trainer is writable as well
    fresh = _trainer(size, seed=4)
    fresh.step(dev(x), truth=truth, ntruth=ntruth)
    net_utils.save_darknet_weights(fresh, str(tmp_path / "fresh.weights"), BATCH)
    assert net_utils.load_darknet_weights(_detector(size), str(tmp_path / "fresh.weights")) == BATCH


def test_load_darknet_prefix_fills_the_core_without_a_fold(weights_file, tmp_path):
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    _path, _file_layers, layers = weights_file
    core = str(tmp_path / "narrow.conv.18")
    DW.write(core, layers[:18], 9)
    tr = _trainer(64, seed=6)
    before = [net.export_params() for net in tr.networks()]
    assert net_utils.load_darknet_prefix(tr, core) == 18
    after = [net.export_params() for net in tr.networks()]
    flat_b = [p for net in before for p in net]
    flat_a = [p for net in after for p in net]
    np.testing.assert_array_equal(flat_a[0]["W"], layers[0]["weights"].transpose(2, 3, 1, 0))      # RGB kept, no fold
    np.testing.assert_array_equal(flat_a[0]["moving_mean"], layers[0]["rolling_mean"])
    np.testing.assert_array_equal(flat_a[3]["W"][1, 1], layers[3]["weights"][:, :, 0, 0].T)
    assert not _off_centre(flat_a[3]["W"]).any()
    for l in range(18):
        if l != 3:
            np.testing.assert_array_equal(flat_a[l]["W"], layers[l]["weights"].transpose(2, 3, 1, 0))
        np.testing.assert_array_equal(flat_a[l]["gamma"], layers[l]["scales"])
        np.testing.assert_array_equal(flat_a[l]["beta"], layers[l]["biases"])
        np.testing.assert_array_equal(flat_a[l]["moving_var"], layers[l]["rolling_variance"])
        assert not flat_a[l]["b"].any()
    for l in range(18, 23):
        for k in flat_b[l]:
            assert flat_a[l][k].tobytes() == flat_b[l][k].tobytes(), (l, k)
    # a detector of the topology takes it too; a file that ends inside a layer or fits no prefix is refused
    assert net_utils.load_darknet_prefix(_detector(64), core) == 18
    cut = str(tmp_path / "cut.weights")
    with open(cut, "wb") as f:
        f.write(open(core, "rb").read()[:-8])
    with pytest.raises(ValueError) as e:
        net_utils.load_darknet_prefix(tr, cut)
    assert "inside layer" in str(e.value)
    with pytest.raises(ValueError):
        net_utils.load_darknet_prefix(_trainer(64, num_class=4), weights_file[0])       # 23 layers of another head
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    with pytest.raises(ValueError):
        net_utils.load_darknet_prefix(yolov2.YOLOv2Trainer(BATCH, 64, num_class=NUM_CLASS, dtype="f32",
                                                           width_div=WIDTH_DIV, bn_eps=1e-6), core)


# ---------------------------------------------------------------- 6. the caller
def test_train_caller_fine_tunes_and_resumes_darknet_files(voc_weights_file, tmp_path, golden_dir):
    from test_box_list_host import build_devkit
    from tensorflow_yolo2_amd.pascal import pascal_eval_yolov2, pascal_train_yolov2
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    path, _file_layers, layers = voc_weights_file
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    ckpt = str(tmp_path / "ckpt")
    common = ["--devkit", kit, "--width-div", "8", "--batch", "2", "--size", "64", "--dtype", "f32"]
    first = pascal_train_yolov2.main(common + ["--darknet-weights", path, "--iters", "1", "--ckpt-dir", ckpt])
    assert isinstance(first["trainer"], yolov2.YOLOv2DarknetTrainer) and np.isfinite(np.array(first["losses"])).all()
    assert (first["first_iter"], first["last_iter"]) == (1, 1)
    snap1 = os.path.join(ckpt, "train_iter_1.weights")
    assert DW.read(snap1)[3] == 2
    second = pascal_train_yolov2.main(common + ["--topology", "darknet", "--ckpt-dir", ckpt, "--iters", "1"])
    assert (second["first_iter"], second["last_iter"]) == (2, 2) and second["trainer"].iteration == 2
    snap2 = os.path.join(ckpt, "train_iter_2.weights")
    assert DW.read(snap2)[3] == 4 and open(snap2, "rb").read() != open(snap1, "rb").read()
    res = pascal_eval_yolov2.main(common + ["--image-set", "trainval", "--per-class", "--letterbox",
                                            "--darknet-weights", snap2])
    assert res["detector"].topology == "darknet" and np.isfinite(res["mAP"])
    core = str(tmp_path / "narrow.conv.18")
    DW.write(core, layers[:18], 9)
    third = pascal_train_yolov2.main(common + ["--topology", "darknet", "--darknet-backbone", core, "--iters", "1",
                                               "--box-labels", "--solver", "darknet", "--burn-in", "3"])
    assert isinstance(third["trainer"], yolov2.YOLOv2DarknetTrainer) and np.isfinite(np.array(third["losses"])).all()
    # each topology refuses a directory of the other's snapshots, naming both
    other = str(tmp_path / "paper_ckpt")
    os.makedirs(other)
    open(os.path.join(other, "train_iter_3.npz"), "wb").close()
    with pytest.raises(ValueError) as e:
        pascal_train_yolov2.main(common + ["--topology", "darknet", "--ckpt-dir", other, "--iters", "1"])
    assert "paper" in str(e.value) and "darknet" in str(e.value)
    with pytest.raises(ValueError) as e:
        pascal_train_yolov2.main(common + ["--ckpt-dir", ckpt, "--iters", "1"])
    assert "paper" in str(e.value) and "darknet" in str(e.value)
