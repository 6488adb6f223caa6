"""Device-resident classifier batches on the GPU: y2_warp_u8_batch (csrc/augment.hip) bit for bit against
img_dataset/augment_cls.py for hand-written rows on both of its paths, DeviceCls against the host batcher cls_images batch
by batch, one trainer step from either feed, and the train script's --device-data path.  Everything this feature computes
is compared by equality; the one bound is on the loss scalar of the existing cross-entropy kernel (_same_loss says why)."""
import ctypes as C

import numpy as np
import pytest

from test_cls_augment_host import write_list

pytestmark = pytest.mark.gpu

POOL_SHAPES = [(1, 1), (2, 3), (37, 53), (64, 48), (5, 200), (130, 97), (300, 260)]
LIST_SHAPES = [(40, 52), (64, 48), (33, 33), (90, 70), (37, 53), (50, 120), (32, 32)]
COLOURS = ((0.0, 1.0, 1.0), (0.07, 1.3, 0.8))


def _AC():
    from tensorflow_yolo2_amd.img_dataset import augment_cls
    return augment_cls


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from tensorflow_yolo2_amd import _lib as L
    return L, L.load()


@pytest.fixture(scope="module")
def pool():
    """the 7 images, their pool and table on the device and a label per entry; left unchanged by every test"""
    import torch
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV
    imgs = [np.random.default_rng([77, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in POOL_SHAPES]
    offsets, pitches, total = DV.pool_layout(POOL_SHAPES)
    assert pitches[4] == 608
    host = np.zeros(total, np.uint8)
    for im, off, pitch in zip(imgs, offsets, pitches):
        host[off:off + im.shape[0] * pitch] = DV.padded_rows(im, pitch).reshape(-1)
    table = np.array([(off, h, w, pitch, 1) for (h, w), off, pitch in zip(POOL_SHAPES, offsets, pitches)], np.int64)
    labels = np.array([11, 0, 999, 5, 42, 7, 300], np.int32)       # (the flip column is set: the kernel must not read it)
    return {"imgs": imgs, "table": table, "labels": labels, "pool_d": torch.from_numpy(host).cuda(),
            "table_d": torch.from_numpy(table).cuda(), "labels_d": torch.from_numpy(labels).cuda()}


def _warp(pool, index, rows, out_h, out_w, fill=127, with_labels=True):
    import torch
    L, lib = _lib()
    n = len(index)
    out = torch.full((n, out_h, out_w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    lab = torch.full((n,), -5, dtype=torch.int32, device="cuda") if with_labels else None
    index_d = torch.from_numpy(np.asarray(index, np.int32)).cuda()
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda() if rows is not None else None
    L.check(lib.y2_warp_u8_batch(_ptr(pool["pool_d"]), _ptr(pool["table_d"]), _ptr(index_d), _ptr(rows_d),
                                 _ptr(pool["labels_d"]) if with_labels else None, n, out_h, out_w, fill, _ptr(out),
                                 _ptr(lab), None))
    torch.cuda.synchronize()
    return out.cpu().numpy(), (lab.cpu().numpy() if with_labels else None)


def _cases(size):
    """[(entry, six map values)] written by hand for an output of size x size"""
    AC = _AC()
    cases = [(e, AC.identity_row(h, w, size)[:6]) for e, (h, w) in enumerate(POOL_SHAPES)]
    for e in (2, 6):
        h, w = POOL_SHAPES[e]
        cases.append((e, AC.compose(h, w, size, size, 0, 0, 0.0, True)))                   # mirror
    for e, deg in ((2, 0.0), (3, 7.0), (5, 33.3), (3, 90.0), (5, 180.0), (6, 33.3), (4, 7.0), (0, 33.3), (1, 90.0)):
        h, w = POOL_SHAPES[e]
        sw, sh = (size + 9, int((size + 9) * h / w)) if w <= h else (int((size + 9) * w / h), size + 9)
        sw, sh = max(sw, size), max(sh, size)
        cases.append((e, AC.compose(h, w, sw, sh, (sw - size) // 2, sh - size, deg, deg == 7.0)))
    cases.append((3, np.array([1, 0, 3, 0, 1, -5], np.float64)))        # scale 1, odd offsets: 3 * x is no multiple of 4
    cases.append((5, np.array([1, 0, 7, 0, 1, 11], np.float64)))
    cases.append((2, np.array([1, 0, 5000, 0, 1, 0], np.float64)))      # every tile outside the image
    cases.append((5, np.array([float("nan"), 0, 0, 0, 1, 0], np.float64)))
    cases.append((5, np.array([1, 0, 2.0 ** 31, 0, 1, 0], np.float64)))
    cases.append((6, np.array([2.0 ** 29, 0, 0, 0, 1, 0], np.float64)))     # column 0 alone is a coordinate
    cases.append((6, np.array([0.5, 0, -3.25, 0, 0.5, 250.5], np.float64)))  # up-scaling across the bottom edge
    return cases


def _paths(pool, e, row, size):
    AC = _AC()
    off, h, w, pitch, _ = (int(x) for x in pool["table"][e])
    tiles = (size + AC.TILE - 1) // AC.TILE
    return {AC.tile_path(h, w, pitch, off, row, size, size, tx, ty) for tx in range(tiles) for ty in range(tiles)}


@pytest.mark.parametrize("size", [32, 64])
def test_kernel_equals_the_specification_on_both_paths(pool, size):
    """batches of 5 with a repeated entry; 64 has more than one tile in each direction.  The helper that restates the
    kernel's box-versus-budget rule says which paths ran: the 300 x 260 image stretched to 32 reads the pool in place,
    the 64 x 48 image cropped at scale 1 is staged, the row that leaves the image is fill."""
    AC = _AC()
    cases = _cases(size)
    seen = set()
    for e, m in cases:
        seen |= _paths(pool, e, m, size)
    assert seen == {"staged", "inplace", "fill"}, seen
    if size == 32:
        assert _paths(pool, 6, cases[6][1], 32) == {"inplace"}
        big = pool["table"][6]
        assert big[2] / 32 > 8 and big[1] / 32 > 8
    assert _paths(pool, 3, np.array([1, 0, 3, 0, 1, -5], np.float64), size) <= {"staged", "fill"}
    assert "staged" in _paths(pool, 3, np.array([1, 0, 3, 0, 1, -5], np.float64), size)
    aug = AC.ClsAugment(fill=93)
    for colour in COLOURS:
        for k in range(0, len(cases), 4):
            chunk = cases[k:k + 4]
            chunk = chunk + [chunk[0]] * (5 - len(chunk))               # 5 slots, one entry twice
            index = [e for e, _ in chunk]
            rows = np.array([list(m) + list(colour) for _, m in chunk], np.float64)
            got, lab = _warp(pool, index, rows, size, size, fill=93)
            assert (lab == pool["labels"][index]).all()
            for b, (e, _) in enumerate(chunk):
                want = aug.image(pool["imgs"][e], rows[b], size)
                assert (got[b] == want).all(), (size, colour, k + b, e, rows[b].tolist(),
                                                int((got[b] != want).sum()))


def test_kernel_without_parameters_forms_the_identity_rows(pool):
    AC = _AC()
    for size in (32, 64):
        for index in ([0, 1, 2, 3, 3], [4, 5, 6, 6, 0]):
            got, lab = _warp(pool, index, None, size, size, fill=127)
            assert (lab == pool["labels"][index]).all()
            for b, e in enumerate(index):
                assert (got[b] == AC.plain_image(pool["imgs"][e], size, 127)).all(), (size, e)
    got, lab = _warp(pool, [6, 2], None, 40, 36, with_labels=False)     # a non-square output, no labels
    assert lab is None
    for b, e in enumerate([6, 2]):
        h, w = POOL_SHAPES[e]
        M = AC.compose(h, w, 36, 40, 0, 0, 0.0, False)
        assert (got[b] == AC.warp_affine_u8(pool["imgs"][e], M, 40, 36, 127)).all()


def test_every_refusal_is_an_argument_error_and_writes_nothing(pool):
    import torch
    L, lib = _lib()
    out = torch.full((2 * 32 * 32 * 3 + 4,), 0xA5, dtype=torch.uint8, device="cuda")
    lab = torch.full((2,), -5, dtype=torch.int32, device="cuda")
    index = torch.zeros(2, dtype=torch.int32, device="cuda")
    P, T, LB = _ptr(pool["pool_d"]), _ptr(pool["table_d"]), _ptr(pool["labels_d"])
    O, O1 = _ptr(out), C.c_void_p(out.data_ptr() + 1)
    calls = [
        (P, T, _ptr(index), None, LB, 0, 32, 32, 127, O, _ptr(lab), None),          # n < 1
        (P, T, _ptr(index), None, LB, 2, 0, 32, 127, O, _ptr(lab), None),           # out_h < 1
        (P, T, _ptr(index), None, LB, 2, 32, 0, 127, O, _ptr(lab), None),           # out_w < 4
        (P, T, _ptr(index), None, LB, 2, 32, 30, 127, O, _ptr(lab), None),          # out_w % 4
        (P, T, _ptr(index), None, LB, 2, 32, 32, -1, O, _ptr(lab), None),           # fill
        (P, T, _ptr(index), None, LB, 2, 32, 32, 256, O, _ptr(lab), None),
        (P, T, _ptr(index), None, LB, 2, 32, 32, 127, O1, _ptr(lab), None),         # a misaligned out
        (P, T, _ptr(index), None, None, 2, 32, 32, 127, O, _ptr(lab), None),        # one of labels / labels_out
        (P, T, _ptr(index), None, LB, 2, 32, 32, 127, O, None, None),
    ]
    for args in calls:
        assert lib.y2_warp_u8_batch(*args) == -1, args[5:9]                         # Y2_ERR_ARG
        assert b"y2_warp_u8_batch" in lib.y2_last_error()
    torch.cuda.synchronize()
    assert (out == 0xA5).all() and (lab == -5).all()


# ---- batchers
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_device_cls_equals_the_host_batcher(tmp_path, rank, world):
    """4 batches of 5 from a list of 7 (of 2 under world = 2, crossing the wrap of 3 positions per epoch), plain and
    with the full turn of the reference"""
    import torch
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    AC = _AC()
    items, _ = write_list(tmp_path, LIST_SHAPES)
    batch = 5 if world == 1 else 2
    for aug in (None, AC.ClsAugment(angle=180)):
        dev = DeviceCls(items, batch, seed=4, rank=rank, world=world, augment=aug)
        host = cls_images(items, batch, seed=4, rank=rank, world=world, augment=aug)
        for k in range(4):
            images, labels = dev.get(64)
            torch.cuda.synchronize()
            want_i, want_l = host.get_u8(64)
            assert images.dtype == torch.uint8 and labels.dtype == torch.int32
            assert (images.cpu().numpy() == want_i).all(), (aug, k)
            assert (labels.cpu().numpy() == want_l).all(), (aug, k)


def test_one_pool_serves_two_sizes_and_skips(tmp_path):
    import torch
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    AC = _AC()
    items, _ = write_list(tmp_path, LIST_SHAPES)
    aug = AC.ClsAugment()
    dev = DeviceCls(items, 5, seed=1, augment=aug, pool_short_side=40)
    host = cls_images(items, 5, seed=1, augment=aug, pool_short_side=40)
    assert dev.table.cpu().numpy()[:, 1:3].tolist() == host.shapes.tolist() and host.shapes.min(axis=1).max() == 40
    for size in (32, 64):
        images, labels = dev.get(size)
        torch.cuda.synchronize()
        want_i, want_l = host.get_u8(size)
        assert (images.cpu().numpy() == want_i).all() and (labels.cpu().numpy() == want_l).all(), size
    dev.skip_batches(2)
    host.get_u8(32), host.get_u8(32)
    images, labels = dev.get(64)
    torch.cuda.synchronize()
    want_i, want_l = host.get_u8(64)
    assert (images.cpu().numpy() == want_i).all() and (labels.cpu().numpy() == want_l).all()
    with pytest.raises(ValueError, match="multiple of 32"):
        dev.get(48)
    with pytest.raises(ValueError, match="augment=None"):
        dev.eval_batch(64, 0)
    with pytest.raises(MemoryError, match="bytes"):
        DeviceCls(items, 5, max_pool_bytes=1000)


def test_eval_batch_is_the_plain_stretch_in_list_order(tmp_path):
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    from tensorflow_yolo2_amd.img_dataset.device_images import DeviceImages
    items, _ = write_list(tmp_path, LIST_SHAPES)
    dev = DeviceCls(items, 3)
    ref = DeviceImages([p for p, _ in items], 3)
    for start in (0, 3, 6):
        images, valid = dev.eval_batch(64, start)
        want, want_valid = ref.batch(64, start, letterbox=False)
        torch.cuda.synchronize()
        assert valid == want_valid and (images == want).all()
        idx = np.minimum(np.arange(start, start + 3), 6)
        assert dev.labels_of(start).cpu().numpy().tolist() == [items[i][1] for i in idx]
        assert dev.labels_of(start).dtype == torch.int32


# ---- trainer
def _same_loss(la, lb, n):
    """The loss SCALAR of y2_softmax_cross_entropy is not a function of its input's bits: the kernel adds the n row terms
    with a float32 atomicAdd in arrival order (csrc/loss.hip), and one logits tensor gave 3 different scalars over 200
    calls on the device.  So the scalars of two equal steps are compared within what reordering n positive float32
    terms can do -- n - 1 additions, each rounding by at most half an ulp of a partial sum that does not exceed the total:
    (n - 1) ulp(total) between two orders -- while the logits and the updated parameters, which the scalar does not
    feed, are compared bit for bit by the callers."""
    assert np.isfinite(la) and np.isfinite(lb)
    assert abs(np.float32(la) - np.float32(lb)) <= (n - 1) * np.spacing(np.float32(max(la, lb))), (la, lb)


def test_trainer_step_from_the_pool_equals_the_step_from_uploaded_bytes(tmp_path):
    import torch
    from oracle import nn_ref as R
    from tensorflow_yolo2_amd.img_dataset.cls_images import cls_images
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    from tensorflow_yolo2_amd.trainer import ClassifierTrainer
    AC = _AC()
    items, _ = write_list(tmp_path, LIST_SHAPES)
    core = [(k, ci, co, int(p)) for (k, ci, co, p) in R.scaled_spec(R.CORE_SPEC, 8)]
    spec = core + [(1, core[-1][2], 1000, 0)]
    aug = AC.ClsAugment()
    images, labels = DeviceCls(items, 5, seed=3, augment=aug).get(64)
    want_i, want_l = cls_images(items, 5, seed=3, augment=aug).get_u8(64)
    a = ClassifierTrainer(5, 64, dtype="f32", spec=spec, seed=2)
    b = ClassifierTrainer(5, 64, dtype="f32", spec=spec, seed=2)
    loss_a, logits_a = a.step(images, labels)
    loss_b, logits_b = b.step(torch.from_numpy(want_i).cuda(), torch.from_numpy(want_l).cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(logits_a).all() and torch.equal(logits_a.view(torch.int32), logits_b.view(torch.int32))
    assert torch.equal(a.net.params.view(torch.int32), b.net.params.view(torch.int32))      # after the update
    _same_loss(float(loss_a), float(loss_b), 5)


# ---- script
def test_train_script_from_the_device_pool(tmp_path, monkeypatch, capsys):
    import torch
    from tensorflow_yolo2_amd.imagenet import imagenet_train_darknet
    from tensorflow_yolo2_amd.img_dataset import device_cls
    items, _ = write_list(tmp_path, LIST_SHAPES)
    lst = tmp_path / "train.txt"
    lst.write_text("".join("%s %d\n" % it for it in items))
    argv = ["--image-list", str(lst), "--device-data", "--augment", "--iters", "3", "--batch", "4", "--size", "64",
            "--dtype", "f32"]
    built = []
    real = device_cls.DeviceCls

    def counting(*a, **k):
        built.append(k.get("augment"))
        return real(*a, **k)
    monkeypatch.setattr(device_cls, "DeviceCls", counting)
    r1 = imagenet_train_darknet.main(argv)
    out1 = capsys.readouterr().out
    r2 = imagenet_train_darknet.main(argv)
    assert len(r1["log"]) == 3 and np.isfinite(r1["log"]).all() and len(r2["log"]) == 3
    # two runs: the same training bit for bit (every variable and Momentum slot after the third step), the same
    # accuracies, and loss scalars equal up to the order of the loss kernel's atomic sum (_same_loss)
    assert torch.equal(r1["trainer"].net.params.view(torch.int32), r2["trainer"].net.params.view(torch.int32))
    assert torch.equal(r1["trainer"].opt.accum.view(torch.int32), r2["trainer"].opt.accum.view(torch.int32))
    for (l1, a1), (l2, a2) in zip(r1["log"], r2["log"]):
        assert a1 == a2
        _same_loss(l1, l2, 4)
    assert len(built) == 2 and built[0] is not None and built[0].angle == 7.0
    assert out1.count("training loss") == 3
    # the existing arguments still run the existing code: no pool is built
    del built[:]
    r3 = imagenet_train_darknet.main(["--iters", "1", "--batch", "4", "--size", "64", "--dtype", "f32",
                                      "--image-list", str(lst)])
    assert not built and len(r3["log"]) == 1 and np.isfinite(r3["log"]).all()
    with pytest.raises(SystemExit):
        imagenet_train_darknet.main(["--device-data", "--iters", "1"])
