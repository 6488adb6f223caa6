"""Darknet's shuffle-then-cut of a crowded image's boxes on the host (img_dataset/augment.py: box_rank,
encode_box_list_draw): equality with encode_box_list where nothing is cut, the properties of the cut, the kept frequency
over many keys, and the key stream's independence of the other two streams of a pool.  No GPU."""
import numpy as np
import pytest

from test_box_list_host import OBJS, H, W, build_devkit
from tensorflow_yolo2_amd.img_dataset import augment as A

KEYS = (0, 1, 0x9E3779B9, 0xFFFFFFFF, 123456789)
SIZE = 416


def crowd(n=40, h=480, w=640):
    """n objects of a w x h image whose centres lie inside it, classes 0 .. n - 1 so that a row names its object"""
    rng = np.random.default_rng(11)
    objs = []
    for k in range(n):
        cx, cy = rng.uniform(20, w - 20), rng.uniform(20, h - 20)
        bw, bh = rng.uniform(8, 120), rng.uniform(8, 120)
        objs.append((np.floor(max(1.0, cx - bw / 2)), np.floor(max(1.0, cy - bh / 2)),
                     np.ceil(min(float(w), cx + bw / 2)), np.ceil(min(float(h), cy + bh / 2)), k))
    return objs, h, w


def test_box_rank_is_the_stated_hash():
    def stated(key, j):
        m = 0xFFFFFFFF
        x = (key ^ (j * 0x9E3779B9)) & m
        x ^= x >> 16
        x = (x * 0x7FEB352D) & m
        x ^= x >> 15
        x = (x * 0x846CA68B) & m
        x ^= x >> 16
        return x
    for key in KEYS:
        got = A.box_rank(key, np.arange(200))
        assert got.dtype == np.uint32 and got.tolist() == [stated(key, j) for j in range(200)]
    assert int(A.box_rank(0, 0)) == 0 and int(A.box_rank(7, 3)) == stated(7, 3)
    assert A.box_rank(np.array([1, 2])[:, None], np.arange(3)[None, :]).shape == (2, 3)


def test_at_most_max_boxes_survivors_is_encode_box_list_whatever_the_key():
    windows = (A.identity_row(H, W), A.identity_row(H, W, 1), np.array([60, -10, 292, 270, 0, 0.05, 1.2, 0.9], np.float64),
               np.array([400, 300, 50, 50, 0, 0, 1, 1], np.float64))
    for row in windows:
        for flip in (False, True):
            for T in (5, 30):
                want_t, want_n = A.encode_box_list(OBJS, row, SIZE, T, flip)
                for key in KEYS:
                    got_t, got_n = A.encode_box_list_draw(OBJS, row, SIZE, T, key, flip)
                    assert got_n == want_n and np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    objs, h, w = crowd(30)
    want_t, want_n = A.encode_box_list(objs, A.identity_row(h, w), SIZE, 30)
    for key in KEYS:                                                    # exactly T survivors: still nothing to cut
        got_t, got_n = A.encode_box_list_draw(objs, A.identity_row(h, w), SIZE, 30, key)
        assert got_n == want_n == 30 and np.array_equal(got_t.view(np.uint32), want_t.view(np.uint32))
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            A.encode_box_list_draw(OBJS, A.identity_row(H, W), SIZE, bad, 1)
    for bad_key in (-1, 1 << 32):
        with pytest.raises(ValueError):
            A.encode_box_list_draw(OBJS, A.identity_row(H, W), SIZE, 30, bad_key)


@pytest.mark.parametrize("flip", (False, True))
def test_forty_survivors_cut_to_thirty(flip):
    objs, h, w = crowd(40)
    row = A.identity_row(h, w)
    full, n_full = A.encode_box_list(objs, row, SIZE, 64, flip)
    assert n_full == 40
    chosen = {}
    for key in KEYS:
        truth, count = A.encode_box_list_draw(objs, row, SIZE, 30, key, flip)
        assert truth.shape == (30, 5) and count == 30                   # exactly 30 rows
        kept = [int(c) for c in truth[:, 4]]
        assert kept == sorted(kept) and len(set(kept)) == 30            # annotation order, no object twice
        for r, j in zip(truth, kept):                                   # each row is a row of the uncut list
            assert np.array_equal(r.view(np.uint32), full[j].view(np.uint32))
        again, _ = A.encode_box_list_draw(objs, row, SIZE, 30, key, flip)
        assert np.array_equal(again.view(np.uint32), truth.view(np.uint32))     # the same key, the same rows
        # and they are the 30 smallest (hash, j)
        ranks = A.box_rank(key, np.arange(40))
        assert kept == sorted(sorted(range(40), key=lambda j: (int(ranks[j]), j))[:30])
        chosen[key] = kept
    assert chosen[1] != chosen[0x9E3779B9]                              # two keys of a fixed pair differ
    # the cut is over the SURVIVORS: with a window that drops objects, 30 of those that are left
    row = np.array([int(0.1 * w), 0, int(0.9 * w), h, 0, 0, 1, 1], np.float64)     # the left tenth is cut: 34 are left
    left, n_left = A.encode_box_list(objs, row, SIZE, 64, flip)
    assert 30 < n_left < 40
    truth, count = A.encode_box_list_draw(objs, row, SIZE, 30, 5, flip)
    alive = [int(c) for c in left[:n_left, 4]]
    assert count == 30 and set(int(c) for c in truth[:, 4]) <= set(alive)
    ranks = A.box_rank(5, np.arange(40))
    assert [int(c) for c in truth[:, 4]] == sorted(sorted(alive, key=lambda j: (int(ranks[j]), j))[:30])


def test_every_object_is_kept_three_times_in_four():
    """2,000 keys, 40 survivors, T = 30: every object's kept frequency within 0.75 +- 0.05 -- five standard deviations of
    a binomial with p = 0.75, n = 2,000 (sigma = 0.0097).  Fixed inputs: the keys are the first 2,000 of a seeded key
    stream"""
    objs, h, w = crowd(40)
    rng = A.key_generator(3, 0)
    kept = np.zeros(40)
    for _ in range(2000):
        truth, count = A.encode_box_list_draw(objs, A.identity_row(h, w), SIZE, 30, A.draw_key(rng))
        assert count == 30
        kept[truth[:, 4].astype(int)] += 1
    freq = kept / 2000.0
    print("kept frequency: min %.4f max %.4f" % (freq.min(), freq.max()))
    assert (np.abs(freq - 0.75) <= 0.05).all(), freq


def test_the_draw_moves_neither_the_batch_order_nor_the_augmentation_rows(tmp_path, golden_dir, monkeypatch):
    from tensorflow_yolo2_amd.img_dataset import device_voc as DV
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    monkeypatch.setattr(DV.DeviceVOC, "_alloc_pool", lambda self, n: np.zeros(n, np.uint8))
    monkeypatch.setattr(DV.DeviceVOC, "_put", lambda self, pool, off, flat: None)
    monkeypatch.setattr(DV.DeviceVOC, "_upload", lambda self, a: a)
    kw = dict(batch_size=4, devkit_path=kit, flipped=True, seed=9, augment=A.Augment(), max_boxes=30)
    plain, drawn = DV.DeviceVOC("trainval", **kw), DV.DeviceVOC("trainval", draw=True, **kw)
    other = DV.DeviceVOC("trainval", draw=True, **dict(kw, seed=10))
    keys, other_keys = [], []
    for _ in range(3 * 4):                                              # the samples of the first three batches
        e0, row0, key0 = plain.next_sample()
        e1, row1, key1 = drawn.next_sample()
        assert e0 == e1 and np.array_equal(row0, row1) and key0 is None
        assert isinstance(key1, int) and 0 <= key1 < 1 << 32
        keys.append(key1)
        other_keys.append(other.next_sample()[2])
    assert len(set(keys)) == 12 and keys != other_keys
    again = DV.DeviceVOC("trainval", draw=True, **kw)
    assert [again.next_sample()[2] for _ in range(12)] == keys           # seeded by (seed, rank)
    assert A.KEY_STREAM != A.STREAM
    with pytest.raises(ValueError, match="max_boxes"):
        DV.DeviceVOC("trainval", batch_size=4, devkit_path=kit, draw=True)


def test_train_script_draw_flag_needs_box_labels(capsys):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as T
    with pytest.raises(SystemExit):
        T.parse_args(["--devkit", "x", "--draw-boxes"])
    assert "--box-labels" in capsys.readouterr().err
    assert T.parse_args(["--devkit", "x"]).draw_boxes is False
    assert T.parse_args(["--devkit", "x", "--box-labels"]).draw_boxes is False       # off by default
    assert T.parse_args(["--devkit", "x", "--box-labels", "--draw-boxes"]).draw_boxes is True
