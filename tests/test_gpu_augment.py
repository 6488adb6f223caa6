"""Training augmentation on the GPU: y2_augment_u8_batch and y2_encode_labels_window (csrc/augment.hip) against the plain
kernels of csrc/data.hip for identity rows and bit for bit against img_dataset/augment.py for drawn and hand-written
rows, DeviceVOC(augment=...) against the host batcher batch by batch, and the train script's --augment paths.
Everything here is equality: no tolerance anywhere."""
import ctypes as C
import os

import numpy as np
import pytest

from test_device_voc_host import make_devkit
from test_gpu_device_voc import MULTI_SCALE_SIZES, _lib, _pool, _ptr, _resize, _source_images

pytestmark = pytest.mark.gpu


def _A():
    from tensorflow_yolo2_amd.img_dataset import augment
    return augment


def _augment(pool_d, table_d, index, rows, out_h, out_w, fill=127):
    import torch
    L, lib = _lib()
    n = len(rows)
    out = torch.full((n, out_h, out_w, 3), 0xA5, dtype=torch.uint8, device="cuda")
    index_d = torch.from_numpy(np.asarray(index, np.int32)).cuda() if index is not None else None
    rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
    L.check(lib.y2_augment_u8_batch(_ptr(pool_d), _ptr(table_d), _ptr(index_d) if index is not None else None,
                                    _ptr(rows_d), n, out_h, out_w, fill, _ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _random_objects(rng, shapes, max_obj, beyond=True):
    """per image an object list as tests/test_gpu_device_voc.py draws them: crowded cells, boxes on and (`beyond`) beyond
    the borders -- the centre of the one beyond them lies outside a small image, where the window rule drops it"""
    lists = []
    for k, (ih, iw) in enumerate(shapes):
        cnt = (0, max_obj, 1)[k] if k < 3 else int(rng.integers(4, max_obj + 1))
        objs = []
        for _ in range(cnt):
            x = np.sort(rng.integers(1, iw + 1, 2)).astype(float)
            y = np.sort(rng.integers(1, ih + 1, 2)).astype(float)
            objs.append((x[0], y[0], x[1], y[1], int(rng.integers(0, 20))))
        if cnt >= 4:
            objs[1] = objs[0][:4] + ((objs[0][4] + 3) % 20,)
            objs[2] = (1.0, 1.0, float(iw), float(ih), 5)
            objs[3] = (0.0, -3.0, float(iw + 40), float(ih + 9), 6) if beyond else (1.0, float(ih), float(iw), float(ih), 6)
        lists.append(objs)
    return lists


def _label_tables(lists, table, max_obj):
    """device (boxes, counts) for a table of len(lists) plain entries followed by their flipped copies"""
    import torch
    n = len(table)
    boxes = np.full((n, max_obj, 5), 7.0, np.float64)            # beyond the count: never read
    counts = np.zeros(n, np.int32)
    for k in range(n):
        objs = lists[k % len(lists)]
        counts[k] = len(objs)
        if objs:
            boxes[k, :len(objs)] = np.asarray(objs, np.float64)
    return torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda()


def _labels(window, boxes_d, counts_d, table_d, index, rows, max_obj, size, S):
    import torch
    L, lib = _lib()
    n = len(rows)
    out = torch.full((n, S, S, 25), float("nan"), dtype=torch.float32, device="cuda")
    index_d = torch.from_numpy(np.asarray(index, np.int32)).cuda() if index is not None else None
    ip = _ptr(index_d) if index is not None else None
    if window:
        rows_d = torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda()
        L.check(lib.y2_encode_labels_window(_ptr(boxes_d), _ptr(counts_d), _ptr(table_d), ip, _ptr(rows_d), n, max_obj,
                                            size, S, 20, _ptr(out), None))
    else:
        L.check(lib.y2_encode_labels(_ptr(boxes_d), _ptr(counts_d), _ptr(table_d), ip, n, max_obj, size, S, 20,
                                     _ptr(out), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_identity_rows_equal_the_plain_kernels(golden_dir):
    """the parent's kernels on the same pool: every multi-scale size, 64, 224, a non-square output, one whose rows are
    not a multiple of 4 bytes, and an unaligned pool; all source shapes and both table flips in every launch.  A row
    flip on top equals the plain kernel on the entry with the opposite flip."""
    import torch
    A = _A()
    imgs = _source_images(golden_dir)
    n = 2 * len(imgs)
    ident = np.array([A.identity_row(*imgs[k % len(imgs)].shape[:2]) for k in range(n)])
    mirrored = ident.copy()
    mirrored[:, 4] = 1
    opposite = np.concatenate([np.arange(len(imgs), n), np.arange(len(imgs))]).astype(np.int32)
    for aligned, outputs in ((True, [(s, s) for s in MULTI_SCALE_SIZES + (64, 224)] + [(96, 160), (97, 150)]),
                             (False, [(320, 320), (97, 150)])):
        pool, table = _pool(imgs, aligned=aligned)
        assert aligned or (table[:, 0] % 16 != 0).any()
        pool_d, table_d = torch.from_numpy(pool).cuda(), torch.from_numpy(table).cuda()
        for (oh, ow) in outputs:
            want = _resize(pool_d, table_d, None, n, oh, ow)
            assert np.array_equal(_augment(pool_d, table_d, None, ident, oh, ow), want), (aligned, oh, ow)
            assert np.array_equal(_augment(pool_d, table_d, opposite, mirrored, oh, ow), want), (aligned, oh, ow)
    # labels, for in-image annotations (what lies beyond the image is the window rule's to drop)
    rng = np.random.default_rng(78)
    max_obj = 12
    lists = _random_objects(rng, [im.shape[:2] for im in imgs], max_obj, beyond=False)
    boxes_d, counts_d = _label_tables(lists, table, max_obj)
    index = rng.integers(0, n, 3 * n).astype(np.int32)
    rows = ident[index]
    for S in (2, 10, 13, 19):
        want = _labels(False, boxes_d, counts_d, table_d, index, rows, max_obj, 32 * S, S)
        assert want[:, :, :, 0].sum() > n
        assert np.array_equal(_labels(True, boxes_d, counts_d, table_d, index, rows, max_obj, 32 * S, S), want), S


def _hand_rows(h, w):
    return [(-(w // 2) - 1, -(h // 2) - 2, 2 * w + 3, 2 * h + 5, 0, 0.1, 1.5, 1.5),       # overhangs all four sides
            (w // 2, h // 2, 1, 1, 1, -0.1, 1 / 1.5, 1.5),                                # one pixel
            (w + 5, h + 3, 7, 9, 0, 0.25, 1.2, 0.8),                                      # wholly outside: all fill
            (-20, -20, 10, 10, 1, 0.0, 1.0, 1.0),
            (0, 0, w, h, 0, 0.0, 1000.0, 1000.0),                                         # extreme factors
            (0, 0, w, h, 1, 0.0, 0.001, 0.001),
            (-3, 2, w, h, 0, 0.5, 1.0, 1.0),                                              # half a turn either way
            (3, -2, w, h, 1, -0.5, 1.0, 1.0),
            (0, 0, w, h, 0, 0.0, 1.0, 1.0)]                                               # identity among the others


def test_kernels_equal_the_specification(golden_dir):
    """rows drawn by Augment.draw at jitter 0.3 and the hand-written ones, on every source shape with both table flips;
    every launch mixes shapes, flips and rows, one goes through a permuted index with repeats (all do: the slots pick
    entries) and one through an unaligned pool; images AND label grids equal the host specification bit for bit"""
    import torch
    A = _A()
    imgs = _source_images(golden_dir)
    shapes = [im.shape[:2] for im in imgs]
    m = len(imgs)
    aug, rng = A.Augment(jitter=0.3), A.generator(17, 0)
    lists = _random_objects(np.random.default_rng(79), shapes, 12)
    slots = []                                                    # (entry, row)
    for k in range(m):
        for r in _hand_rows(*shapes[k]):
            slots.append((k + m * (len(slots) % 2), np.array(r, np.float64)))
        for _ in range(3):
            slots.append((k + m * (len(slots) % 2), aug.draw(rng, *shapes[k])))
    order = np.random.default_rng(3).permutation(len(slots))      # shapes, flips and rows interleaved
    slots = [slots[i] for i in order] + [slots[order[0]], slots[order[5]], slots[order[0]]]      # with repeats
    index = np.array([e for e, _ in slots], np.int32)
    rows = np.array([r for _, r in slots])
    assert len(set(index.tolist())) == 2 * m and (rows[:, 4] == 1).any() and (rows[:, 4] == 0).any()
    pool, table = _pool(imgs)
    pool_d, table_d = torch.from_numpy(pool).cuda(), torch.from_numpy(table).cuda()
    pool_u, table_u = _pool(imgs, aligned=False)
    boxes_d, counts_d = _label_tables(lists, table, 12)
    for (oh, ow, fill) in ((416, 416, 127), (64, 64, 127), (97, 150, 0), (352, 352, 255)):
        spec = A.Augment(fill=fill)
        want = [spec.image(imgs[e % m], r, oh, ow, flip=e >= m) for e, r in slots]
        got = _augment(pool_d, table_d, index, rows, oh, ow, fill)
        for k in range(len(slots)):
            assert np.array_equal(got[k], want[k]), (oh, ow, int(index[k]), rows[k].tolist())
        if (oh, ow) in ((64, 64), (97, 150)):
            got = _augment(torch.from_numpy(pool_u).cuda(), torch.from_numpy(table_u).cuda(), index, rows, oh, ow, fill)
            assert np.array_equal(got, np.stack(want)), (oh, ow, "unaligned")
    kept = dropped = 0
    for S in (2, 13, 19):
        size = 32 * S
        got = _labels(True, boxes_d, counts_d, table_d, index, rows, 12, size, S)
        for k, (e, r) in enumerate(slots):
            want = A.encode_boxes_window(lists[e % m], r, size, S, flip=e >= m).astype(np.float32)
            assert np.array_equal(got[k], want), (S, int(e), r.tolist())
            kept += int(want[:, :, 0].sum())
            dropped += int(want[:, :, 0].sum() == 0 and len(lists[e % m]) > 0)
    assert kept > 100 and dropped > 3


def test_argument_errors():
    import torch
    L, lib = _lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    table = torch.tensor([[0, 4, 4, 16, 0]], dtype=torch.int64, device="cuda")
    rows = torch.tensor([[0, 0, 4, 4, 0, 0, 1, 1]], dtype=torch.float64, device="cuda")
    for (n, oh, ow, fill) in ((0, 8, 8, 127), (1, 0, 8, 127), (1, 8, 0, 127), (1, 1, 1025, 127), (1, 8, 8, -1), (1, 8, 8, 256)):
        assert lib.y2_augment_u8_batch(_ptr(buf), _ptr(table), None, _ptr(rows), n, oh, ow, fill, _ptr(buf), None) < 0
        assert b"y2_augment_u8_batch" in lib.y2_last_error()
    for args in ((None, _ptr(table), _ptr(rows), _ptr(buf)), (_ptr(buf), None, _ptr(rows), _ptr(buf)),
                 (_ptr(buf), _ptr(table), None, _ptr(buf)), (_ptr(buf), _ptr(table), _ptr(rows), None)):
        assert lib.y2_augment_u8_batch(args[0], args[1], None, args[2], 1, 8, 8, 127, args[3], None) < 0
        assert b"null" in lib.y2_last_error()
    boxes = torch.zeros(5, dtype=torch.float64, device="cuda")
    counts = torch.zeros(1, dtype=torch.int32, device="cuda")
    for (n, max_obj, size, S) in ((0, 1, 64, 2), (1, 0, 64, 2), (1, 1, 0, 2), (1, 1, 64, 0)):
        assert lib.y2_encode_labels_window(_ptr(boxes), _ptr(counts), _ptr(table), None, _ptr(rows), n, max_obj, size, S, 20,
                                           _ptr(buf), None) < 0
        assert b"y2_encode_labels_window" in lib.y2_last_error()
    assert lib.y2_encode_labels_window(_ptr(boxes), _ptr(counts), _ptr(table), None, None, 1, 1, 64, 2, 20, _ptr(buf), None) < 0
    # a row without a window is no argument error (the rows live on the device): that slot is all fill, its grid empty
    empty = torch.tensor([[0, 0, 0, 4, 0, 0.1, 1.5, 1.5], [0, 0, 4, float("nan"), 0, 0, 1, 1]], dtype=torch.float64, device="cuda")
    two = torch.tensor([[0, 4, 4, 16, 0], [0, 4, 4, 16, 1]], dtype=torch.int64, device="cuda")
    out = torch.full((2, 8, 7, 3), 0xA5, dtype=torch.uint8, device="cuda")
    assert lib.y2_augment_u8_batch(_ptr(buf), _ptr(two), None, _ptr(empty), 2, 8, 7, 9, _ptr(out), None) == 0
    grid = torch.full((2, 2, 2, 25), float("nan"), dtype=torch.float32, device="cuda")
    boxes2 = torch.tensor([[1, 1, 4, 4, 3]] * 2, dtype=torch.float64, device="cuda")
    counts2 = torch.ones(2, dtype=torch.int32, device="cuda")
    assert lib.y2_encode_labels_window(_ptr(boxes2), _ptr(counts2), _ptr(two), None, _ptr(empty), 2, 1, 64, 2, 20, _ptr(grid), None) == 0
    torch.cuda.synchronize()
    assert (out == 9).all() and (grid == 0).all()
    # the legal call next to them works
    assert lib.y2_augment_u8_batch(_ptr(buf), _ptr(table), None, _ptr(rows), 1, 8, 8, 127, _ptr(buf[1024:]), None) == 0
    torch.cuda.synchronize()


def test_augmented_device_batches_equal_the_host_batchers_sequence(tmp_path, golden_dir):
    """two epochs, flipped copies on, world 1 and both ranks of world 2: the k-th get(size) is the k-th get_u8()"""
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    A = _A()
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=3)          # 4 images, 8 entries
    firsts = {}
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        for size in (64, 320, 416):
            kw = dict(batch_size=4, devkit_path=kit, flipped=True, seed=11, rank=rank, world=world, augment=A.Augment())
            ds = DeviceVOC("trainval", **kw)
            host = pascal_voc("trainval", image_size=size, cell_size=size // 32, **kw)
            assert ds.per_rank == 8 // world
            for b in range(2 * ds.per_rank // 4):
                images, labels = ds.get(size)
                torch.cuda.synchronize()
                want_i, want_l = host.get_u8()
                assert images.dtype == torch.uint8 and labels.dtype == torch.float32
                assert np.array_equal(images.cpu().numpy(), want_i), (rank, world, size, b)
                assert np.array_equal(labels.cpu().numpy(), want_l), (rank, world, size, b)
                assert ds.cursor == host.cursor
                if b == 0:
                    firsts[(rank, world, size)] = want_i
    assert not np.array_equal(firsts[(0, 2, 64)], firsts[(1, 2, 64)])             # each rank its own shard and draws
    # against the plain batch of the same order: augmented, and not everywhere
    plain = pascal_voc("trainval", image_size=64, cell_size=2, batch_size=4, devkit_path=kit, flipped=True, seed=11)
    assert not np.array_equal(plain.get_u8()[0], firsts[(0, 1, 64)])


def test_no_host_pixel_work_after_start_up_with_augmentation(tmp_path, golden_dir, monkeypatch):
    import torch
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV, pascal_voc as PV
    A = _A()
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir)
    ds = DV.DeviceVOC("trainval", batch_size=3, devkit_path=kit, flipped=True, seed=2, augment=A.Augment())

    def boom(*a, **k):
        raise AssertionError("host pixel work after start-up")
    for mod in (DV, PV):
        monkeypatch.setattr(mod, "imread_bgr", boom)
    for mod in (PV, A):
        monkeypatch.setattr(mod, "resize_bilinear_u8", boom)
    for name in ("crop_resize_u8", "distort_hsv_u8", "encode_boxes_window"):
        monkeypatch.setattr(A, name, boom)
    with pytest.raises(AssertionError, match="host pixel work"):
        PV.pascal_voc("trainval", batch_size=3, devkit_path=kit, image_size=64, augment=A.Augment()).get_u8()   # (the patch bites)
    seen = []
    for s in (64, 96, 128, 64):
        images, labels = ds.get(s)
        torch.cuda.synchronize()
        assert images.shape == (3, s, s, 3) and labels.shape == (3, s // 32, s // 32, 25)
        assert images.cpu().numpy().std() > 10 and torch.isfinite(labels).all()
        seen.append(images.cpu().numpy())
    assert not np.array_equal(seen[0], seen[3])


def test_train_script_with_augmentation(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.pascal import pascal_train_darknet
    from tensorflow_yolo2_amd.yolo2_nets import darknet
    kit = make_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=3)
    ms = ["--devkit", kit, "--augment", "--multi-scale", "--ms-sizes", "64,96,128", "--ms-period", "2", "--iters", "6",
          "--batch", "4", "--dtype", "f32"]
    one = ["--iters", "3", "--batch", "4", "--size", "64", "--dtype", "f32", "--devkit", kit, "--flipped"]
    darknet.reset_default_graph()
    try:
        r1 = pascal_train_darknet.main(ms)
        assert len(r1["losses"]) == 6 and np.isfinite(r1["losses"]).all()
        assert len(set(r1["sizes"])) > 1 and set(r1["sizes"]) <= {64, 96, 128}
        darknet.reset_default_graph()
        fed = pascal_train_darknet.main(one + ["--augment"])
        darknet.reset_default_graph()
        dev = pascal_train_darknet.main(one + ["--augment", "--device-data"])
        assert fed["losses"] == dev["losses"] and np.isfinite(fed["losses"]).all()
        darknet.reset_default_graph()
        plain = pascal_train_darknet.main(one)
        assert plain["losses"][0] != fed["losses"][0]                      # (the flag does something)
    finally:
        darknet.reset_default_graph()
        darknet.set_default_dtype("f16")


def test_augmented_multi_scale_two_ranks_on_one_gpu(tmp_path, golden_dir):
    """the data-parallel entry point with --augment: each rank draws for its own shard, nothing is exchanged, and the
    ranks end with bit-identical variables and Adam slots (tests/dp_train_worker.py checks that on the device tensors)"""
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
           "--batch", "4", "--dtype", "f32", "--ckpt-dir", ck, "--devkit", kit, "--flipped", "--augment", "--multi-scale",
           "--ms-sizes", "64,96", "--ms-period", "1", "--all-ranks-on-gpu0", "--dist-backend", "gloo"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert "dp-train ok last_iter=4" in r.stdout, r.stdout[-2000:]
    assert os.path.exists(os.path.join(ck, "train_iter_4.npz"))
