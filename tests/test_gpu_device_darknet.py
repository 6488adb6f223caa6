"""Training and evaluation batches from a Darknet image list on the GPU (img_dataset/device_boxes.py: DeviceDarknet) and
from a COCO instances file (device_coco.py: DeviceCOCOTrain): bit-equal to the host specification applied slot by slot,
with and without an Augment and the draw; the same images as a VOC devkit and as a list; the list-order batch."""
import os
import shutil

import numpy as np
import pytest

from test_box_list_host import build_devkit
from test_darknet_data_host import _devkit_as_list, _ulp_apart
from tensorflow_yolo2_amd.img_dataset import augment as A
from tensorflow_yolo2_amd.utils import darknet_data as DD

gpu = pytest.mark.gpu
CLASSES = 3
# label rows per image: 0, 1, 2, 3 and 9 objects, and again 2 -- with max_boxes = 4 the fifth image is cut
LABELS = ([],
          [(0, 0.5, 0.5, 0.4, 0.5)],
          [(1, 0.3, 0.4, 0.2, 0.3), (2, 0.7, 0.6, 0.25, 0.2)],
          [(2, 0.2, 0.2, 0.1, 0.1), (2, 0.21, 0.22, 0.12, 0.1), (0, 0.8, 0.7, 0.3, 0.4)],
          [(k % 3, 0.1 + 0.09 * k, 0.15 + 0.08 * k, 0.08 + 0.01 * k, 0.1) for k in range(9)],
          [(0, 0.6, 0.3, 0.3, 0.2), (1, 0.4, 0.75, 0.5, 0.3)])
CROPS = ((0, 0, 120, 90), (30, 20, 131, 97), (100, 50, 164, 146), (10, 10, 170, 74), (0, 100, 200, 228), (150, 0, 240, 100))


def make_list(root, golden_dir):
    """six small PNG crops of testImg1 under root/images with their label files -> the list file"""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"))
    paths = []
    with Image.open(os.path.join(golden_dir, "testImg1.jpg")) as im:
        im = im.convert("RGB")
        for k, (box, rows) in enumerate(zip(CROPS, LABELS)):
            p = os.path.join(root, "images", "im%d.png" % k)
            im.crop(box).save(p)
            DD.write_labels(DD.label_path(p), rows)
            paths.append(p)
    lst = os.path.join(root, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst


@gpu
@pytest.mark.parametrize("augment", (False, True))
@pytest.mark.parametrize("draw", (False, True))
def test_device_darknet_batches_equal_the_host_specification(tmp_path, golden_dir, augment, draw):
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_boxes import DeviceDarknet
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import imread_bgr, resize_bilinear_u8
    lst = make_list(str(tmp_path), golden_dir)
    size, T, B = 96, 4, 4
    kw = dict(batch_size=B, flipped=True, seed=3, max_boxes=T, draw=draw)
    aug = lambda: A.Augment() if augment else None
    ds, twin = DeviceDarknet(lst, CLASSES, augment=aug(), **kw), DeviceDarknet(lst, CLASSES, augment=aug(), **kw)
    assert ds.num_class == 3 and ds.classes == ("0", "1", "2") and len(ds.entries) == 6 and ds.max_obj == 9
    assert ds.counts.cpu().tolist() == [len(r) for r in LABELS] * 2 and not ds.difficult.cpu().numpy().any()
    assert ds.image_index == ["im%d" % k for k in range(6)]
    cut = 0
    for batch in range(3):
        got = [t.cpu().numpy() for t in ds.get(size)]
        torch.cuda.synchronize()
        assert [g.shape for g in got] == [(B, size, size, 3), (B, 3, 3, 5 + CLASSES), (B, T, 5), (B,)]
        for slot in range(B):
            entry, row, key = twin.next_sample()
            e, flip = ds.entries[entry % 6], entry >= 6
            img = imread_bgr(e['imname'])
            if augment:
                want_img = A.Augment().image(img, row, size, size, flip=flip)
            else:
                row = A.identity_row(*e['shape'])
                want_img = resize_bilinear_u8(img, size, size)
                want_img = want_img[:, ::-1, :] if flip else want_img
            want_grid = A.encode_boxes_window(e['objs'], row, size, size // 32, CLASSES, flip).astype(np.float32)
            if draw:
                assert key == int(ds.last_keys[slot])
                want_t, want_n = A.encode_box_list_draw(e['objs'], row, size, T, key, flip)
                cut += int(A.encode_box_list(e['objs'], row, size, 64, flip)[1] > T)
            else:
                assert key is None
                want_t, want_n = A.encode_box_list(e['objs'], row, size, T, flip)
            what = (batch, slot, entry)
            assert np.array_equal(got[0][slot], want_img), what
            assert np.array_equal(got[1][slot], want_grid), what
            assert np.array_equal(got[2][slot].view(np.uint32), want_t.view(np.uint32)), what
            assert got[3][slot] == want_n, what
    if draw and not augment:
        assert cut > 0                                          # the crowded image was drawn at least once in 12 samples


@gpu
def test_a_devkit_and_its_darknet_list_give_the_same_batches(tmp_path, golden_dir):
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_boxes import DeviceDarknet
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=2)
    lst, _entries = _devkit_as_list(kit, str(tmp_path / "dk"))
    size = 96
    voc = DeviceVOC("trainval", batch_size=3, devkit_path=kit, flipped=False, seed=5, max_boxes=30)
    dk = DeviceDarknet(lst, 20, batch_size=3, seed=5, max_boxes=30)
    for _ in range(2):
        a, b = [t.cpu().numpy() for t in voc.get(size)], [t.cpu().numpy() for t in dk.get(size)]
        torch.cuda.synchronize()
        assert np.array_equal(a[0], b[0])                           # the same images in the same order
        assert np.array_equal(a[3], b[3]) and a[3].min() >= 1       # ntruth
        assert np.array_equal(a[2][:, :, 4], b[2][:, :, 4])         # the class column
        worst = int(_ulp_apart(np.ascontiguousarray(a[2][:, :, :4]), np.ascontiguousarray(b[2][:, :, :4])).max())
        print("box columns: at most %d ulp apart" % worst)
        assert worst <= 1
    # the list-order batch is DeviceVOC's
    voc_e = DeviceVOC("trainval", batch_size=2, devkit_path=kit, flipped=False)
    dk_e = DeviceDarknet(lst, 20, batch_size=2)
    for start in (0, 2):
        for kw in (dict(), dict(letterbox=True, fill=100), dict(letterbox=True, protocol="darknet")):
            (ia, va), (ib, vb) = voc_e.eval_batch(size, start, **kw), dk_e.eval_batch(size, start, **kw)
            assert va == vb == min(2, 3 - start) and torch.equal(ia, ib) and torch.equal(voc_e.eval_index, dk_e.eval_index)
    assert torch.equal(voc_e.counts, dk_e.counts) and torch.equal(voc_e.table, dk_e.table)
    with pytest.raises(ValueError, match="DeviceDarknet"):
        DeviceDarknet(lst, 20, batch_size=2, flipped=True).eval_batch(size, 0)
    with pytest.raises(ValueError, match="names"):
        DeviceDarknet(lst, 20, names=("a", "b"), batch_size=2)


@gpu
def test_coco_training_pool_runs_on_the_tiny_instances_file(golden_dir):
    import torch
    from tensorflow_yolo2_amd.img_dataset.device_coco import DeviceCOCOTrain
    ds = DeviceCOCOTrain(os.path.join(golden_dir, "coco", "instances_tiny.json"), golden_dir, 2, seed=1,
                         augment=A.Augment(), max_boxes=2, draw=True)
    assert ds.num_class == 3 and ds.classes == ("person", "car", "cat") and ds.category_ids == [1, 3, 17]
    assert ds.image_ids == [7, 19, 42] and ds.counts.cpu().tolist() == [3, 0, 3] and ds.max_obj == 3
    assert tuple(ds.boxes.shape) == (3, 3, 5) and tuple(ds.table.shape) == (3, 5)
    for _ in range(3):
        images, labels, truth, ntruth = ds.get(96)
        torch.cuda.synchronize()
        assert tuple(images.shape) == (2, 96, 96, 3) and tuple(labels.shape) == (2, 3, 3, 8)
        assert tuple(truth.shape) == (2, 2, 5) and ntruth.dtype == torch.int32
        n = ntruth.cpu().numpy()
        assert ((0 <= n) & (n <= 2)).all()
        for slot in range(2):
            assert not truth[slot, int(n[slot]):].cpu().numpy().any()
            assert set(truth[slot, :int(n[slot]), 4].cpu().tolist()) <= {0.0, 1.0, 2.0}
