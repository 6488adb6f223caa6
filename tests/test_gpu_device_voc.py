"""Device-resident VOC batches on the GPU: y2_resize_bilinear_u8_batch and y2_encode_labels (csrc/data.hip) bit for bit
against oracle/data_ref.py, DeviceVOC against the host batcher batch by batch, and the train script's --device-data /
--multi-scale paths.  Everything here is equality: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import data_ref as D
from test_device_voc_host import make_devkit

pytestmark = pytest.mark.gpu

MULTI_SCALE_SIZES = tuple(range(320, 609, 32))
AWKWARD_SHAPES = ((1, 1), (1, 7), (7, 1), (333, 500), (500, 375), (37, 1024), (5, 1400))   # (height, width)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _lib():
    from tensorflow_yolo2_amd import _lib as L
    return L, L.load()


def _source_images(golden_dir):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import imread_bgr
    rng = np.random.default_rng(2024)
    imgs = [imread_bgr(os.path.join(golden_dir, "testImg1.jpg")), imread_bgr(os.path.join(golden_dir, "testImg2.jpg"))]
    assert imgs[0].shape == (240, 352, 3) and imgs[1].shape == (500, 353, 3)
    return imgs + [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w) in AWKWARD_SHAPES]


def _pool(imgs, aligned=True):
    """(pool uint8, table int64 [2 * len][5]): every image plain, then every image flipped"""
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV
    if aligned:
        offsets, pitches, total = DV.pool_layout([im.shape[:2] for im in imgs])
    else:                                   # tightly packed from byte 1: nothing is 16-byte aligned
        pitches = [3 * im.shape[1] for im in imgs]
        offsets = (1 + np.concatenate([[0], np.cumsum([im.shape[0] * p for im, p in zip(imgs, pitches)])])).tolist()
        total, offsets = offsets[-1], offsets[:-1]
    pool = np.zeros(total, np.uint8)
    for im, off, pitch in zip(imgs, offsets, pitches):
        pool[off:off + im.shape[0] * pitch] = DV.padded_rows(im, pitch).reshape(-1)
    table = np.array([(off, im.shape[0], im.shape[1], pitch, flip)
                      for flip in (0, 1) for im, off, pitch in zip(imgs, offsets, pitches)], np.int64)
    return pool, table


def _resize(pool_d, table_d, index_d, n, out_h, out_w):
    import torch
    L, lib = _lib()
    out = torch.full((n, out_h, out_w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    L.check(lib.y2_resize_bilinear_u8_batch(_ptr(pool_d), _ptr(table_d), _ptr(index_d) if index_d is not None else None,
                                            n, out_h, out_w, _ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_resize_is_bit_equal_to_the_host_resize(golden_dir):
    """both fixture images and random images of awkward shapes (1 x 1 ... 37 x 1024, and 5 x 1400 whose rows are wider
    than the kernel stages) to every multi-scale size, 64, 224 and two non-square outputs (one with a row length that
    is not a multiple of 4 bytes): up- and down-scaling, flip on and off.  EVERY launch mixes all the source shapes with
    both flips in one batch; one more goes through a permuted index and one through an unaligned pool."""
    import torch
    imgs = _source_images(golden_dir)
    pool, table = _pool(imgs)
    assert (table[:, 0] % 16 == 0).all() and (table[:, 3] % 16 == 0).all()
    pool_d, table_d = torch.from_numpy(pool).cuda(), torch.from_numpy(table).cuda()
    n = len(table)
    outputs = [(s, s) for s in MULTI_SCALE_SIZES + (64, 224)] + [(96, 160), (97, 150)]
    want = {}
    for (oh, ow) in outputs:
        ref = [D.resize_bilinear_u8(im, oh, ow) for im in imgs]
        want[(oh, ow)] = np.stack(ref + [r[:, ::-1, :] for r in ref])
        got = _resize(pool_d, table_d, None, n, oh, ow)
        assert got.shape == want[(oh, ow)].shape
        for k in range(n):
            assert np.array_equal(got[k], want[(oh, ow)][k]), (oh, ow, tuple(table[k, 1:3]), int(table[k, 4]))
    # a permuted index with repeats
    index = np.random.default_rng(1).integers(0, n, 2 * n).astype(np.int32)
    got = _resize(pool_d, table_d, torch.from_numpy(index).cuda(), len(index), 416, 416)
    assert np.array_equal(got, want[(416, 416)][index])
    # a pool without any alignment: read in place, same bytes
    pool_u, table_u = _pool(imgs, aligned=False)
    assert (table_u[:, 0] % 16 != 0).any()
    for (oh, ow) in ((320, 320), (97, 150)):
        got = _resize(torch.from_numpy(pool_u).cuda(), torch.from_numpy(table_u).cuda(), None, n, oh, ow)
        assert np.array_equal(got, want[(oh, ow)])


def test_resize_and_label_argument_errors():
    import torch
    L, lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0, 4, 4, 16, 0]], dtype=torch.int64, device="cuda")
    for (n, oh, ow) in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 1, 1025)):
        assert lib.y2_resize_bilinear_u8_batch(_ptr(buf), _ptr(table), None, n, oh, ow, _ptr(buf), None) < 0
        assert b"y2_resize_bilinear_u8_batch" in lib.y2_last_error()
    assert lib.y2_resize_bilinear_u8_batch(None, _ptr(table), None, 1, 8, 8, _ptr(buf), None) < 0
    boxes = torch.zeros(5, dtype=torch.float64, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    for (n, max_obj, size, S) in ((0, 1, 64, 2), (1, 0, 64, 2), (1, 1, 0, 2), (1, 1, 64, 0)):
        assert lib.y2_encode_labels(_ptr(boxes), _ptr(counts), _ptr(table), None, n, max_obj, size, S, 20, _ptr(buf), None) < 0
        assert b"y2_encode_labels" in lib.y2_last_error()
    torch.cuda.synchronize()


def _encode(entries, max_obj, image_size, S):
    """entries: [(objs, im_h, im_w, flip)] -> labels [n, S, S, 25] float32 from the kernel"""
    import torch
    L, lib = _lib()
    n = len(entries)
    boxes = np.zeros((n, max_obj, 5), np.float64)
    counts = np.zeros(n, np.int32)
    table = np.zeros((n, 5), np.int64)
    for k, (objs, h, w, flip) in enumerate(entries):
        counts[k] = len(objs)
        if objs:
            boxes[k, :len(objs)] = np.asarray(objs, np.float64)
        boxes[k, len(objs):] = 7.0                          # beyond the count: never read
        table[k] = (0, h, w, 0, flip)
    out = torch.full((n, S, S, 25), float("nan"), dtype=torch.float32, device="cuda")
    b, c, t = torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(table).cuda()
    L.check(lib.y2_encode_labels(_ptr(b), _ptr(c), _ptr(t), None, n, max_obj, image_size, S, 20, _ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _want_label(objs, h, w, flip, image_size, S):
    lab = D.encode_boxes(objs, h, w, image_size, S)
    if flip:
        from tensorflow_yolo2_amd.img_dataset.pascal_voc import flip_label
        lab = flip_label(lab, image_size)
    return lab.astype(np.float32)


def test_labels_are_bit_equal_to_the_host_encoder(golden_dir):
    w, h, objs = D.parse_voc_xml(open(os.path.join(golden_dir, "testImg2Anno.xml")).read())
    g = np.load(os.path.join(golden_dir, "label_grid_testImg2.npz"))
    for size, S, key in ((224, 7, "grid_224_7"), (416, 13, "grid_416_13")):
        got = _encode([(objs, h, w, 0), (objs, h, w, 1)], len(objs), size, S)
        assert np.array_equal(got[0], g[key].astype(np.float32))
        assert np.array_equal(got[0], _want_label(objs, h, w, 0, size, S))
        assert np.array_equal(got[1], _want_label(objs, h, w, 1, size, S))
    # random object lists: crowded cells (first wins), boxes on and beyond every border (the clamp), 0 and max_obj objects
    rng = np.random.default_rng(77)
    max_obj = 12
    for S in (10, 13, 19):
        size = 32 * S
        entries = []
        for case in range(12):
            ih, iw = int(rng.integers(100, 501)), int(rng.integers(100, 501))
            cnt = (0, max_obj, 1)[case] if case < 3 else int(rng.integers(4, max_obj + 1))
            objs_k = []
            for _ in range(cnt):
                x = np.sort(rng.integers(1, iw + 1, 2)).astype(float)
                y = np.sort(rng.integers(1, ih + 1, 2)).astype(float)
                objs_k.append((x[0], y[0], x[1], y[1], int(rng.integers(0, 20))))
            if cnt >= 4:
                objs_k[1] = objs_k[0][:4] + ((objs_k[0][4] + 3) % 20,)                 # the same cell twice: first wins
                objs_k[2] = (1.0, 1.0, float(iw), float(ih), 5)                         # touches all four borders
                objs_k[3] = (0.0, -3.0, float(iw + 40), float(ih + 9), 6)               # beyond them: clamped
            for flip in (0, 1):
                entries.append((objs_k, ih, iw, flip))
        got = _encode(entries, max_obj, size, S)
        crowded = 0
        for k, (objs_k, ih, iw, flip) in enumerate(entries):
            want = _want_label(objs_k, ih, iw, flip, size, S)
            assert np.array_equal(got[k], want), (S, k)
            crowded += int(want[:, :, 0].sum() < len(objs_k))
            if not objs_k:
                assert not got[k].any()
        assert crowded == 20                                 # every list of four or more has a cell that two objects claim


def _equal_batches(ds, host, size, batches):
    import torch
    for b in range(batches):
        images, labels = ds.get(size)
        torch.cuda.synchronize()
        want_i, want_l = host.get_u8()
        assert images.dtype == torch.uint8 and labels.dtype == torch.float32
        assert np.array_equal(images.cpu().numpy(), want_i), (size, b)
        assert np.array_equal(labels.cpu().numpy(), want_l), (size, b)
        assert ds.cursor == host.cursor


def test_device_batches_equal_the_host_batchers_sequence(tmp_path, golden_dir):
    """two epochs, flipped copies on, world 1 and both ranks of world 2: the k-th get(size) is the k-th get_u8()"""
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=3)          # 4 images, 8 entries
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        for size in (64, 320, 416):
            ds = DeviceVOC("trainval", batch_size=4, devkit_path=kit, flipped=True, seed=11, rank=rank, world=world)
            host = pascal_voc("trainval", batch_size=4, devkit_path=kit, image_size=size, cell_size=size // 32,
                              flipped=True, seed=11, rank=rank, world=world)
            assert ds.per_rank == 8 // world
            _equal_batches(ds, host, size, 2 * ds.per_rank // 4)


def test_no_host_pixel_work_after_start_up(tmp_path, golden_dir, monkeypatch):
    import torch
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV, pascal_voc as PV
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir)
    ds = DV.DeviceVOC("trainval", batch_size=3, devkit_path=kit, flipped=True, seed=2)

    def boom(*a, **k):
        raise AssertionError("host pixel work after start-up")
    for mod in (DV, PV):
        monkeypatch.setattr(mod, "imread_bgr", boom)
    monkeypatch.setattr(PV, "resize_bilinear_u8", boom)
    assert not hasattr(DV, "resize_bilinear_u8")
    with pytest.raises(AssertionError, match="host pixel work"):
        PV.pascal_voc("trainval", batch_size=3, devkit_path=kit, image_size=64).get_u8()     # (the patch bites)
    for s in (64, 96, 128, 64):
        images, labels = ds.get(s)
        torch.cuda.synchronize()
        assert images.shape == (3, s, s, 3) and labels.shape == (3, s // 32, s // 32, 25)
        assert images.cpu().numpy().std() > 10 and labels[:, :, :, 0].sum().item() >= 3


def test_train_step_from_device_batch_equals_the_host_fed_step(tmp_path, golden_dir):
    """one f32 detector step at 224 x 224: same kernels, equal inputs -> the same grid and loss, bit for bit"""
    import torch
    from oracle import nn_ref as R
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir)
    n, size, S = 2, 224, 7
    ds = DeviceVOC("trainval", batch_size=n, devkit_path=kit, flipped=True, seed=0)
    host = pascal_voc("trainval", batch_size=n, devkit_path=kit, image_size=size, cell_size=S, flipped=True, seed=0)
    u8, labels = host.get_u8()
    dimg, dlab = ds.get(size)
    spec = E.CORE_SPEC + E.det_head_spec(30)
    net = E.Network(spec, n, size, size, dtype="f32", core_layers=18, training=True)
    net.load_params(R.init_params(spec, seed=0))
    out = []
    for images, lab in ((torch.as_tensor(u8).cuda(), torch.as_tensor(labels).cuda()), (dimg, dlab)):
        grid = net.forward(images, True, True)
        loss, ious, mask, dnet = E.yolo_loss(grid, lab, 20, n, size, S, 2)
        out.append((grid.clone(), loss.clone(), dnet.clone()))
    torch.cuda.synchronize()
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert torch.isfinite(out[0][1]).all() and float(out[0][1][4]) > 0
    net.backward(out[1][2])
    E.AdamOptimizer(net).step()
    assert torch.isfinite(net.params).all()


def test_train_script_multi_scale_and_device_data(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.pascal import pascal_train_darknet
    from tensorflow_yolo2_amd.yolo2_nets import darknet
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=3)
    ck = str(tmp_path / "ckpts")
    ms = ["--devkit", kit, "--multi-scale", "--ms-sizes", "64,96,128", "--ms-period", "2", "--iters", "6", "--batch", "4",
          "--dtype", "f32", "--ckpt-dir", ck]
    darknet.reset_default_graph()
    try:
        r1 = pascal_train_darknet.main(ms)
        assert len(r1["losses"]) == 6 and np.isfinite(r1["losses"]).all()
        assert len(r1["sizes"]) == 6 and len(set(r1["sizes"])) > 1 and set(r1["sizes"]) <= {64, 96, 128}
        assert r1["sizes"] == [pascal_train_darknet.step_size(pascal_train_darknet.parse_args(ms), i) for i in range(1, 7)]
        assert os.path.isfile(os.path.join(ck, "train_iter_6.npz")) and r1["optimizer"].t == 6
        darknet.reset_default_graph()
        r2 = pascal_train_darknet.main(ms)
        assert r2["first_iter"] == 7 and r2["last_iter"] == 12 and r2["optimizer"].t == 12
        assert np.isfinite(r2["losses"]).all() and os.path.isfile(os.path.join(ck, "train_iter_12.npz"))
        # synthetic data at the step's size
        darknet.reset_default_graph()
        r3 = pascal_train_darknet.main(["--multi-scale", "--ms-sizes", "64,96", "--ms-period", "1", "--iters", "4",
                                        "--batch", "2", "--dtype", "f32"])
        assert np.isfinite(r3["losses"]).all() and set(r3["sizes"]) == {64, 96}
        # --device-data at one size: the host-fed run's losses exactly
        one = ["--iters", "3", "--batch", "4", "--size", "64", "--dtype", "f32", "--devkit", kit, "--flipped"]
        darknet.reset_default_graph()
        fed = pascal_train_darknet.main(one)
        darknet.reset_default_graph()
        dev = pascal_train_darknet.main(one + ["--device-data"])
        assert fed["losses"] == dev["losses"] and fed["sizes"] == dev["sizes"] == [64, 64, 64]
    finally:
        darknet.reset_default_graph()
        darknet.set_default_dtype("f16")


def test_multi_scale_device_data_two_ranks_on_one_gpu(tmp_path, golden_dir):
    """the data-parallel entry point with --multi-scale --devkit: both ranks build the pool, agree on the list (the
    start-up check runs: a process group exists), draw the same sizes, read different shards, and end with
    bit-identical variables and Adam slots (tests/dp_train_worker.py checks that on the device tensors)"""
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=5)
    ck = str(tmp_path / "ckpts")
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "Y2_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "dp_train_worker.py"), "--iters", "4",
           "--batch", "4", "--dtype", "f32", "--ckpt-dir", ck, "--devkit", kit, "--flipped", "--multi-scale",
           "--ms-sizes", "64,96", "--ms-period", "1", "--all-ranks-on-gpu0", "--dist-backend", "gloo"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert "dp-train ok last_iter=4" in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(ck, "train_iter_4.npz"))
