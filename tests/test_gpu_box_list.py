"""Box-list labels on the GPU: y2_encode_box_list (csrc/augment.hip) bit-equal to augment.encode_box_list on a hand-built
box table, and DeviceVOC(..., max_boxes=T).get(size) equal to the host batcher's get_u8() on all four arrays."""
import ctypes as C

import numpy as np
import pytest

from test_box_list_host import build_devkit
from tensorflow_yolo2_amd.img_dataset import augment as A

gpu = pytest.mark.gpu
MAX_OBJ = 70
COUNTS = (0, 1, 64, 65, 70)
SHAPES = ((375, 500), (500, 353), (240, 352), (333, 500), (480, 640))        # (height, width) of the five entries
FLIPS = (0, 1, 0, 1, 1)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def box_table():
    """five entries with 0, 1, 64, 65 and 70 objects: the x centres rise with the annotation index, and the middle of
    every list sits near the bottom of its image, so a window can drop the start, the end or the middle of a list"""
    rng = np.random.default_rng(21)
    table = np.zeros((5, 5), np.int64)
    boxes = np.zeros((5, MAX_OBJ, 5), np.float64)
    for e, ((h, w), cnt) in enumerate(zip(SHAPES, COUNTS)):
        table[e] = (0, h, w, (3 * w + 15) // 16 * 16, FLIPS[e])
        for o in range(cnt):
            xc = (o + 0.5) / cnt * w
            middle = cnt // 3 <= o < 2 * cnt // 3
            yc = rng.uniform(0.85, 0.95) * h if middle else rng.uniform(0.1, 0.5) * h
            bw, bh = rng.uniform(4, 0.2 * w), rng.uniform(4, 0.2 * h)
            boxes[e, o] = (np.floor(max(1.0, xc - bw / 2)), np.floor(max(1.0, yc - bh / 2)),
                           np.ceil(min(float(w), xc + bw / 2)), np.ceil(min(float(h), yc + bh / 2)), rng.integers(0, 20))
    return table, boxes, np.asarray(COUNTS, np.int32)


def windows(index, table):
    """one parameter row per batch slot: the start, the middle or the end of the slot's list leaves the window"""
    rows = np.zeros((len(index), A.ROW), np.float64)
    for slot, e in enumerate(index):
        h, w = int(table[e, 1]), int(table[e, 2])
        kind = slot % 3
        if kind == 0:
            rows[slot] = (int(0.3 * w), -7, int(0.8 * w), h + 20, slot & 1, 0.03, 1.2, 0.8)      # the left 30 % is cut
        elif kind == 1:
            rows[slot] = (-11, 0, int(0.7 * w), int(0.8 * h), 1, -0.05, 0.9, 1.1)                # the right and the bottom
        else:
            rows[slot] = (0, -5, w, int(0.75 * h), 0, 0, 1, 1)                                   # the bottom: the middle
    return rows


def host_lists(boxes, counts, table, index, rows, size, T):
    truth = np.zeros((len(index), T, 5), np.float32)
    ntruth = np.zeros(len(index), np.int32)
    kept = []
    for slot, e in enumerate(index):
        objs = [tuple(b) for b in boxes[e, :counts[e]]]
        row = A.identity_row(int(table[e, 1]), int(table[e, 2])) if rows is None else rows[slot]
        truth[slot], ntruth[slot] = A.encode_box_list(objs, row, size, T, flip=bool(table[e, 4]))
        alone = [A.encode_box_list([o], row, size, 1, flip=bool(table[e, 4]))[1] for o in objs]
        kept.append(np.asarray(alone, bool))
    return truth, ntruth, kept


@gpu
@pytest.mark.parametrize("size", (96, 608))
def test_encode_box_list_is_bit_equal_to_the_host_encoder(size):
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    table, boxes, counts = box_table()
    index = np.array([4, 2, 0, 3, 1], np.int32)
    rows = windows(index, table)
    td, bd, cd = (torch.from_numpy(a).cuda() for a in (table, boxes, counts))
    idx, rd = torch.from_numpy(index).cuda(), torch.from_numpy(rows).cuda()
    # the windows do what they were built for on the long lists: objects leave at the start, the middle and the end
    _, _, kept = host_lists(boxes, counts, table, index, rows, size, MAX_OBJ)
    assert not kept[0][:5].any() and kept[0][-5:].all()                 # slot 0 (70 objects): the start is dropped
    assert not kept[3][:5].any() and kept[3][25:40].all()               # slot 3 (65 objects): the same
    assert kept[1][:5].all() and not kept[1][-5:].any()                 # slot 1 (64 objects): the end ...
    assert not kept[1][64 // 3 + 1:2 * 64 // 3 - 1].any()               # ... and the middle of the list
    for T in (1, 30, 70):
        for use_index, params in ((True, None), (True, rd), (False, None), (False, rd)):
            order = index if use_index else np.arange(5, dtype=np.int32)
            want_t, want_n, _ = host_lists(boxes, counts, table, order, None if params is None else rows, size, T)
            truth = torch.full((5, T, 5), -1.0, dtype=torch.float32, device="cuda")
            ntruth = torch.full((5,), -1, dtype=torch.int32, device="cuda")
            _lib.check(lib.y2_encode_box_list(_ptr(bd), _ptr(cd), _ptr(td), _ptr(idx) if use_index else None, _ptr(params),
                                              5, MAX_OBJ, size, T, _ptr(truth), _ptr(ntruth), None))
            got_t, got_n = truth.cpu().numpy(), ntruth.cpu().numpy()
            assert got_n.tolist() == want_n.tolist(), (T, use_index, params is not None)
            assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)), (T, use_index, params is not None)
            if params is None:
                assert got_n.tolist() == [min(T, int(counts[e])) for e in order]
            elif T == 70 and use_index:                          # (the rows were cut for the slots of `index`)
                assert (got_n[np.asarray(counts)[order] >= 64] < 64).all()       # the windows dropped objects
    # argument errors name the call
    buf, cnt = torch.zeros((5, 1030, 5), device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    for args in ((None, _ptr(cd), _ptr(td), None, None, 5, MAX_OBJ, size, 30, _ptr(buf), _ptr(cnt), None),
                 (_ptr(bd), _ptr(cd), _ptr(td), None, None, 5, MAX_OBJ, size, 30, _ptr(buf), None, None),
                 (_ptr(bd), _ptr(cd), _ptr(td), None, None, 0, MAX_OBJ, size, 30, _ptr(buf), _ptr(cnt), None),
                 (_ptr(bd), _ptr(cd), _ptr(td), None, None, 5, MAX_OBJ, size, 0, _ptr(buf), _ptr(cnt), None),
                 (_ptr(bd), _ptr(cd), _ptr(td), None, None, 5, MAX_OBJ, size, 1025, _ptr(buf), _ptr(cnt), None)):
        assert lib.y2_encode_box_list(*args) < 0
        assert b"y2_encode_box_list" in lib.y2_last_error()
    torch.cuda.synchronize()


@gpu
@pytest.mark.parametrize("mode", ("plain", "flipped", "augment"))
def test_device_batches_with_box_lists_equal_the_host_batcher(tmp_path, golden_dir, mode):
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    for size in (320, 416):
        kw = dict(batch_size=2, devkit_path=kit, flipped=(mode == "flipped"), seed=7)
        aug = lambda: A.Augment() if mode == "augment" else None
        ds = DeviceVOC("trainval", max_boxes=30, augment=aug(), **kw)
        host = pascal_voc("trainval", image_size=size, cell_size=size // 32, max_boxes=30, augment=aug(),
                          cache_images=False, **kw)
        more = 0
        for k in range(3):
            got = ds.get(size)
            torch.cuda.synchronize()
            want = host.get_u8()
            assert len(got) == len(want) == 4
            for name, g, w in zip(("images", "labels", "truth", "ntruth"), got, want):
                g = g.cpu().numpy()
                assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape)
                assert np.array_equal(g, w), (mode, size, k, name)
            more += int((want[3] > (want[1][..., 0] == 1).sum(axis=(1, 2))).sum())
        if mode != "augment":
            assert more > 0                                     # the list kept an object that the grid lost
    pair = DeviceVOC("trainval", batch_size=2, devkit_path=kit, seed=7).get(320)
    assert len(pair) == 2 and pair[0].dtype == torch.uint8 and tuple(pair[1].shape) == (2, 10, 10, 25)
    with pytest.raises(ValueError):
        DeviceVOC("trainval", batch_size=2, devkit_path=kit, max_boxes=1025)
