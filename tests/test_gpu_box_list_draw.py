"""The box list with Darknet's shuffle-then-cut on the GPU: y2_encode_box_list_draw (csrc/augment.hip) bit-equal to
augment.encode_box_list_draw on the hand-built table of test_gpu_box_list.py -- 70 objects span two ballot rounds, so the
second round and the rank across rounds are exercised -- with and without windows, for three keys per slot; keys = NULL
against y2_encode_box_list; zero rows beyond ntruth; the argument errors."""
import numpy as np
import pytest

from test_gpu_box_list import MAX_OBJ, _ptr, box_table, windows
from tensorflow_yolo2_amd.img_dataset import augment as A

gpu = pytest.mark.gpu
SIZE = 96
INDEX = np.array([4, 2, 0, 3, 1], np.int32)                     # slots of 70, 64, 0, 65 and 1 objects
KEYS = np.array([[0, 1, 0x9E3779B9, 0xFFFFFFFF, 77],            # three keys per slot
                 [0xDEADBEEF, 2, 3, 4, 5],
                 [123456789, 987654321, 42, 0x80000000, 0x7FFFFFFF]], np.uint32)


def host_lists(boxes, counts, table, rows, T, keys):
    truth = np.zeros((len(INDEX), T, 5), np.float32)
    ntruth = np.zeros(len(INDEX), np.int32)
    survivors = []
    for slot, e in enumerate(INDEX):
        objs = [tuple(b) for b in boxes[e, :counts[e]]]
        row = A.identity_row(int(table[e, 1]), int(table[e, 2])) if rows is None else rows[slot]
        truth[slot], ntruth[slot] = A.encode_box_list_draw(objs, row, SIZE, T, int(keys[slot]), flip=bool(table[e, 4]))
        survivors.append(A.encode_box_list(objs, row, SIZE, MAX_OBJ, flip=bool(table[e, 4]))[1])
    return truth, ntruth, survivors


@gpu
@pytest.mark.parametrize("T", (1, 4, 30, 64, 70))
def test_encode_box_list_draw_is_bit_equal_to_the_host_specification(T):
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    table, boxes, counts = box_table()
    rows = windows(INDEX, table)
    td, bd, cd = (torch.from_numpy(a).cuda() for a in (table, boxes, counts))
    idx, rd = torch.from_numpy(INDEX).cuda(), torch.from_numpy(rows).cuda()
    drawn = 0
    for params in (None, rd):
        plain_t = torch.full((5, T, 5), -7.0, dtype=torch.float32, device="cuda")
        plain_n = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.y2_encode_box_list(_ptr(bd), _ptr(cd), _ptr(td), _ptr(idx), _ptr(params), 5, MAX_OBJ, SIZE, T,
                                          _ptr(plain_t), _ptr(plain_n), None))
        for keys in (None,) + tuple(KEYS):
            kd = None if keys is None else torch.from_numpy(keys.view(np.int32).copy()).cuda()
            truth = torch.full((5, T, 5), -7.0, dtype=torch.float32, device="cuda")       # the sentinel
            ntruth = torch.full((5,), -7, dtype=torch.int32, device="cuda")
            _lib.check(lib.y2_encode_box_list_draw(_ptr(bd), _ptr(cd), _ptr(td), _ptr(idx), _ptr(params), _ptr(kd), 5,
                                                   MAX_OBJ, SIZE, T, _ptr(truth), _ptr(ntruth), None))
            got_t, got_n = truth.cpu().numpy(), ntruth.cpu().numpy()
            what = (T, params is not None, None if keys is None else keys.tolist())
            if keys is None:                                        # the existing call's result
                assert np.array_equal(got_n, plain_n.cpu().numpy()), what
                assert np.array_equal(got_t.view(np.uint32), plain_t.cpu().numpy().view(np.uint32)), what
                continue
            want_t, want_n, survivors = host_lists(boxes, counts, table, None if params is None else rows, T, keys)
            assert got_n.tolist() == want_n.tolist() == [min(T, s) for s in survivors], what
            assert np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32)), what
            for slot in range(5):                                   # zero at and beyond ntruth: no sentinel is left
                assert not got_t[slot, got_n[slot]:].any(), what
            # where a slot holds more survivors than T, the key and not the annotation order decided
            drawn += sum(1 for slot in range(5) if survivors[slot] > T
                         and not np.array_equal(got_t[slot], plain_t.cpu().numpy()[slot]))
    if T < 64:
        assert drawn > 0
    torch.cuda.synchronize()


@gpu
def test_encode_box_list_draw_argument_errors_name_the_call():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    table, boxes, counts = box_table()
    td, bd, cd = (torch.from_numpy(a).cuda() for a in (table, boxes, counts))
    kd = torch.zeros(5, dtype=torch.int32, device="cuda")
    buf, cnt = torch.zeros((5, 1030, 5), device="cuda"), torch.zeros(5, dtype=torch.int32, device="cuda")
    b, c, t, k, o, n = _ptr(bd), _ptr(cd), _ptr(td), _ptr(kd), _ptr(buf), _ptr(cnt)
    for args in ((b, c, t, None, None, k, 5, MAX_OBJ, SIZE, 30, None, n, None),            # null truth
                 (b, c, t, None, None, k, 0, MAX_OBJ, SIZE, 30, o, n, None),               # n = 0
                 (b, c, t, None, None, k, 5, MAX_OBJ, SIZE, 0, o, n, None),                # max_boxes = 0
                 (b, c, t, None, None, k, 5, MAX_OBJ, SIZE, 1025, o, n, None),             # max_boxes = 1025
                 (b, c, t, None, None, k, 5, 1025, SIZE, 30, o, n, None),                  # max_obj beyond Y2_DRAW_MAX_OBJ
                 (b, c, t, None, None, None, 5, 1025, SIZE, 30, o, n, None)):              # ... with or without keys
        assert lib.y2_encode_box_list_draw(*args) == -1                                    # Y2_ERR_ARG
        assert b"y2_encode_box_list_draw" in lib.y2_last_error()
    torch.cuda.synchronize()
