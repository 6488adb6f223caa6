"""The region loss on box lists on the GPU: y2_yolov2_loss_boxes (csrc/ext.hip) against the float64 specification
(utils/region_loss.py) and against the grid-label kernel on collision-free lists, YOLOv2Trainer.step on box lists, and
pascal_train_yolov2 --box-labels with its resume.

Float32 and float64 may decide differently at a tie (noobject threshold, best anchor, cell of a truth), so every parity
input asserts on the CPU, before the device call, that all three decision margins of the float64 specification are at
least 1e-5 -- two orders above float32 IoU rounding.  The seeds below were fixed so that this holds."""
import os

import numpy as np
import pytest

from test_box_list_host import build_devkit
from tensorflow_yolo2_amd.utils import region_loss as RL

gpu = pytest.mark.gpu
MARGIN = 1e-5
VOC = ((1.3221, 1.73145), (3.19275, 4.00944), (5.05587, 8.09892), (9.47112, 4.84053), (11.2364, 10.0071))
THREE = ((1.0, 1.5), (2.5, 3.0), (5.0, 4.0))
NONDEFAULT = dict(coord_scale=2.0, object_scale=3.0, noobject_scale=0.5, class_scale=1.5, thresh=0.4)
# (n, S, B, C, anchors, seed, index of an image left without truths or None)
SHAPES = {"n3_S5": (3, 5, 5, 20, VOC, 11, 1), "n2_S13": (2, 13, 5, 20, VOC, 12, None), "n1_S19": (1, 19, 5, 20, VOC, 13, None),
          "n2_S8_B3_C4": (2, 8, 3, 4, THREE, 14, None)}


def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def parity_input(key):
    """(net, truth [n][30][5], ntruth, anchors, size): image 0 carries 30 truths, several per cell; the others a few"""
    n, S, B, C, anchors, seed, empty = SHAPES[key]
    rng = np.random.default_rng(seed)
    size = 32 * S
    net = (rng.standard_normal((n, S, S, B, 5 + C)) * 0.7).astype(np.float32)
    truth = np.zeros((n, 30, 5), np.float32)
    ntruth = np.zeros(n, np.int32)
    an = np.asarray(anchors)
    for i in range(n):
        k = 30 if i == 0 else (0 if i == empty else int(rng.integers(2, 6)))
        which = rng.integers(0, B, k)
        scale = rng.uniform(0.75, 1.3, (k, 2))
        hot = rng.integers(0, S, (4, 2))                       # image 0: most centres fall into four cells
        cell = hot[rng.integers(0, 4, k)] if i == 0 else rng.integers(0, S, (k, 2))
        centre = (cell + rng.uniform(0.05, 0.95, (k, 2))) * 32.0
        truth[i, :k, 0:2] = centre
        truth[i, :k, 2:4] = np.minimum(an[which] * scale * 32.0 * S / 13.0 if B == 5 else an[which] * scale * 32.0, size - 1.0)
        truth[i, :k, 4] = rng.integers(0, C, k)
        ntruth[i] = k
    return net, truth, ntruth, anchors, size


def checked_reference(net, truth, ntruth, anchors, size, **kw):
    """the float64 specification with its margins asserted: the input decides nothing within 1e-5 of a tie"""
    loss, dnet, m = RL.yolov2_loss_boxes(net, truth, ntruth, anchors, size, dtype=np.float64, return_margins=True, **kw)
    assert m["best_thresh"] >= MARGIN and m["shape_gap"] >= MARGIN and m["cell_edge"] >= MARGIN, m
    return loss, dnet


def assert_close(loss, dnet, ref_loss, ref_d):
    """the project's tolerance for this loss (tests/test_ext.py::test_gpu_yolov2_loss_matches_specification)"""
    print("loss", loss, "reference", ref_loss)
    np.testing.assert_allclose(loss, ref_loss, rtol=2e-5)
    if dnet is not None:
        err = np.abs(dnet - ref_d).max() / np.abs(ref_d).max()
        print("largest gradient error / largest gradient", err)
        assert err < 2e-5, err


@gpu
@pytest.mark.parametrize("key", sorted(SHAPES))
def test_loss_boxes_matches_the_float64_specification(key):
    from tensorflow_yolo2_amd import engine as E
    net, truth, ntruth, anchors, size = parity_input(key)
    n, S, B, C = SHAPES[key][:4]
    assert ntruth[0] == 30
    cells = {(int(t[1] // 32), int(t[0] // 32)) for t in truth[0]}
    assert len(cells) < 15                                              # several truths per cell
    # default scales
    ref_loss, ref_d = checked_reference(net, truth, ntruth, anchors, size)
    loss, dnet = E.yolov2_loss_boxes(dev(net), dev(truth), dev(ntruth), anchors, size)
    assert tuple(dnet.shape) == net.shape
    assert_close(loss.cpu().numpy(), dnet.cpu().numpy(), ref_loss, ref_d)
    # two calls on the same input: the same bits
    loss_b, dnet_b = E.yolov2_loss_boxes(dev(net), dev(truth), dev(ntruth), anchors, size)
    assert np.array_equal(loss.cpu().numpy().view(np.uint32), loss_b.cpu().numpy().view(np.uint32))
    assert np.array_equal(dnet.cpu().numpy().view(np.uint32), dnet_b.cpu().numpy().view(np.uint32))
    # other scales, the area weight and the prior
    ref2, refd2 = checked_reference(net, truth, ntruth, anchors, size, area_weight=True, prior_scale=0.01, **NONDEFAULT)
    sc = dict(NONDEFAULT, area_weight=1.0, prior_scale=0.01)
    l2, d2 = E.yolov2_loss_boxes(dev(net), dev(truth), dev(ntruth), anchors, size, scales=sc)
    assert_close(l2.cpu().numpy(), d2.cpu().numpy(), ref2, refd2)
    assert (np.abs(ref2 - ref_loss) > 1e-3 * np.abs(ref_loss)).all()             # (the scale set changed every part)
    # forward only
    l3, d3 = E.yolov2_loss_boxes(dev(net), dev(truth), dev(ntruth), anchors, size, need_grad=False, scales=sc)
    assert d3 is None
    assert np.array_equal(l3.cpu().numpy().view(np.uint32), l2.cpu().numpy().view(np.uint32))
    # rows beyond ntruth are not read
    dirty = truth.copy()
    for i in range(n):
        dirty[i, ntruth[i]:] = 123.0
    l4, _ = E.yolov2_loss_boxes(dev(net), dev(dirty), dev(ntruth), anchors, size, need_grad=False)
    assert np.array_equal(l4.cpu().numpy().view(np.uint32), loss.cpu().numpy().view(np.uint32))


@gpu
@pytest.mark.parametrize("n,S", [(3, 5), (2, 13), (1, 19)])
def test_loss_boxes_equals_the_grid_kernel_on_collision_free_lists(n, S):
    from tensorflow_yolo2_amd import engine as E, synthetic
    size = 32 * S
    rng = np.random.default_rng(70 + S)
    net = (rng.standard_normal((n, S, S, 5, 25)) * 0.7).astype(np.float32)
    lab = synthetic.det_labels(n, size, S, 80 + S)
    if n > 2:
        lab[1] = 0
    truth, ntruth = RL.grid_to_box_list(lab, 30)
    checked_reference(net, truth, ntruth, VOC, size)
    for sc_grid, sc_list in ((None, None), (NONDEFAULT, NONDEFAULT)):
        g_loss, g_d = E.yolov2_loss(dev(net), dev(lab), VOC, size, scales=sc_grid)
        loss, dnet = E.yolov2_loss_boxes(dev(net), dev(truth), dev(ntruth), VOC, size, scales=sc_list)
        assert_close(loss.cpu().numpy(), dnet.cpu().numpy(), g_loss.cpu().numpy().astype(np.float64),
                     g_d.cpu().numpy().astype(np.float64))


@gpu
def test_loss_boxes_rejects_bad_arguments():
    import ctypes as C
    import torch
    from tensorflow_yolo2_amd import _lib, engine as E
    lib = _lib.load()
    net, truth, ntruth, anchors, size = parity_input("n3_S5")
    p = lambda t: C.c_void_p(t.data_ptr())
    nd, td, cd, ad = dev(net), dev(truth), dev(ntruth), dev(np.asarray(anchors, np.float32))
    loss = torch.empty(5, device="cuda")
    ws = torch.empty(lib.y2_yolov2_loss_boxes_workspace_bytes(3, 5, 5), dtype=torch.uint8, device="cuda")
    call = lambda **kw: lib.y2_yolov2_loss_boxes(*[kw.get(k, v) for k, v in (
        ("net", p(nd)), ("truth", p(td)), ("ntruth", p(cd)), ("anchors", p(ad)), ("batch", 3), ("S", 5), ("B", 5), ("C", 20),
        ("T", 30), ("size", 160.0), ("scales", None), ("loss", p(loss)), ("dnet", None), ("ws", p(ws)), ("stream", None))])
    assert call() == 0
    for kw, word in ((dict(truth=None), b"null"), (dict(ntruth=None), b"null"), (dict(ws=None), b"null"),
                     (dict(T=1025), b"max_boxes"), (dict(T=0), b"max_boxes"), (dict(S=1024, B=2), b"MAX_SLOTS"),
                     (dict(batch=0), b"batch")):
        assert call(**kw) < 0, kw
        assert b"y2_yolov2_loss_boxes" in lib.y2_last_error() and word in lib.y2_last_error(), lib.y2_last_error()
    assert lib.y2_yolov2_loss_boxes_workspace_bytes(3, 1024, 2) == 0
    with pytest.raises(ValueError):
        E.yolov2_loss_boxes(nd, td, cd, anchors, size, scales=dict(coord=1.0))
    # a class index outside [0, C): the row takes no class term, everything else stands (documented contract)
    bad = truth.copy()
    bad[2, 0, 4] = 99.0
    l_bad, d_bad = E.yolov2_loss_boxes(nd, dev(bad), cd, anchors, size)
    r_bad, rd_bad = checked_reference(net, bad, ntruth, anchors, size)
    assert_close(l_bad.cpu().numpy(), d_bad.cpu().numpy(), r_bad, rd_bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the trainer
def two_in_one_cell(n=2, size=96):
    """per image: two objects in cell (1, 1) of the 3 x 3 grid whose shapes are 1.05 x anchors 0 and 1, as a box list and
    as the grid label of the same objects (which keeps the first alone)"""
    S = size // 32
    truth = np.zeros((n, 30, 5), np.float32)
    lab = np.zeros((n, S, S, 25), np.float32)
    for i in range(n):
        truth[i, 0] = (1.3 * 32, 1.6 * 32, 1.05 * VOC[0][0] * 32, 1.05 * VOC[0][1] * 32, 3 + i)
        truth[i, 1] = (1.7 * 32, 1.4 * 32, 1.05 * VOC[1][0] * 32, 1.05 * VOC[1][1] * 32, 9 + i)
        lab[i, 1, 1, 0] = 1
        lab[i, 1, 1, 1:5] = truth[i, 0, :4]
        lab[i, 1, 1, 5 + 3 + i] = 1
    return truth, np.full(n, 2, np.int32), lab


@gpu
def test_trainer_step_on_box_lists_trains_both_objects_of_a_cell():
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, size = 2, 96
    x = dev(synthetic.images(n, size, 31))
    truth, ntruth, lab = two_in_one_cell(n, size)
    td, cd, ld = dev(truth), dev(ntruth), dev(lab)
    tr = yolov2.YOLOv2Trainer(n, size, dtype="f32", seed=3, width_div=8)
    with pytest.raises(ValueError):
        tr.step(x, ld, truth=td, ntruth=cd)
    with pytest.raises(ValueError):
        tr.step(x)
    with pytest.raises(ValueError):
        tr.step(x, truth=td)
    assert tr.iteration == 0
    losses = [float(tr.step(x, truth=td, ntruth=cd)[4])]
    d = tr.last_dnet.cpu().numpy()
    assert np.abs(d[:, 1, 1, 0, :4]).min() > 0 and np.abs(d[:, 1, 1, 1, :4]).min() > 0       # both slots learn
    assert not d[:, 1, 1, 2:, :4].any() and not d[:, 0, :, :, :4].any()                       # no prior by default
    grid = yolov2.YOLOv2Trainer(n, size, dtype="f32", seed=3, width_div=8)
    grid.step(x, ld)
    dg = grid.last_dnet.cpu().numpy()
    assert np.abs(dg[:, 1, 1, 0, :4]).min() > 0 and not dg[:, 1, 1, 1, :4].any()             # the grid label lost the second
    np.testing.assert_allclose(dg[:, 1, 1, 0, :4], d[:, 1, 1, 0, :4], rtol=1e-5)             # ... and kept the first as it was
    losses += [float(tr.step(x, truth=td, ntruth=cd)[4]) for _ in range(4)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    for net in tr.nets:
        assert torch.isfinite(net.params).all()


@gpu
def test_trainer_step_on_box_lists_f16_and_area_weight():
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, size = 2, 96
    x = dev(synthetic.images(n, size, 31))
    truth, ntruth, _ = two_in_one_cell(n, size)
    tr = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=3, width_div=8, area_weight=True)
    losses = [float(tr.step(x, truth=dev(truth), ntruth=dev(ntruth))[4]) for _ in range(5)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    for net in tr.nets:
        assert torch.isfinite(net.params).all()


@gpu
def test_trainer_prior_switches_off_at_the_documented_iteration():
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    n, size = 2, 96
    x = dev(synthetic.images(n, size, 31))
    truth, ntruth, _ = two_in_one_cell(n, size)
    td, cd = dev(truth), dev(ntruth)
    tr = yolov2.YOLOv2Trainer(n, size, dtype="f32", seed=3, width_div=8, prior_images=4)
    assert [tr.prior_on(i) for i in (1, 2, 3, 4)] == [True, True, False, False]    # (i - 1) * 2 images seen < 4
    free = np.ones((n, 3, 3, 5), bool)
    free[:, 1, 1, :2] = False
    coord = []
    for i in (1, 2, 3):
        loss = tr.step(x, truth=td, ntruth=cd)
        d = tr.last_dnet.cpu().numpy()
        assert np.isfinite(float(loss[4])) and np.abs(d[~free][:, :4]).min() > 0
        coord.append(np.abs(d[free][:, :4]))
    assert coord[0].min() > 0 and coord[1].min() > 0 and not coord[2].any()
    # a resumed trainer counts from its snapshot's iteration
    tr2 = yolov2.YOLOv2Trainer(n, size, dtype="f32", seed=3, width_div=8, prior_images=4)
    tr2.iteration = 2
    assert not tr2.prior_on() and tr2.box_scales()["prior_scale"] == 0.0


# ---------------------------------------------------------------- the train script
def _train(kit, ckpt, iters):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2
    return pascal_train_yolov2.main(["--devkit", kit, "--ckpt-dir", ckpt, "--box-labels", "--area-weight", "--prior-images",
                                     "8", "--iters", str(iters), "--batch", "2", "--size", "96", "--width-div", "8",
                                     "--augment"])


def _largest_difference(a, b):
    assert sorted(a.files) == sorted(b.files)
    worst = 0.0
    for k in a.files:
        if a[k].size and not np.array_equal(a[k], b[k]):
            worst = max(worst, float(np.nanmax(np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)))))
    return worst


@gpu
def test_train_script_box_labels_resumes_bitwise(tmp_path, golden_dir):
    """4 iterations in one run against 2, a snapshot, a fresh process state from --ckpt-dir and 2 more (DESIGN.md section
    9's comparison): bitwise against the uninterrupted run.  A second uninterrupted run is the control."""
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    dirs = [str(tmp_path / d) for d in ("whole", "control", "resumed")]
    whole = _train(kit, dirs[0], 4)
    _train(kit, dirs[1], 4)
    first = _train(kit, dirs[2], 2)
    second = _train(kit, dirs[2], 2)
    assert (first["first_iter"], first["last_iter"], second["first_iter"], second["last_iter"]) == (1, 2, 3, 4)
    assert second["trainer"].iteration == 4 and second["trainer"].prior_on(4) and not second["trainer"].prior_on(5)
    assert whole["imdb"].max_boxes == 30 and whole["trainer"].area_weight
    losses = np.array(whole["losses"])
    assert losses.shape == (4, 5) and np.isfinite(losses).all()
    snaps = [np.load(os.path.join(d, "train_iter_4.npz")) for d in dirs]
    control = _largest_difference(snaps[0], snaps[1])
    resumed = _largest_difference(snaps[0], snaps[2])
    print("box-label resume: control run-to-run difference %.3e, resumed difference %.3e" % (control, resumed))
    assert control == 0.0, "the uninterrupted run is not reproducible itself: %.3e" % control
    assert resumed == 0.0
    assert np.array_equal(np.array(first["losses"] + second["losses"]).view(np.uint32), losses.view(np.uint32))
