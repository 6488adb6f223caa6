"""Box-list labels of the anchor model on the host (img_dataset/augment.encode_box_list): every row against the grid cell
the same object wins in encode_boxes / encode_boxes_window, the host batcher's four-array batches on a temporary
devkit, and the train script's flags.  No GPU."""
import os
import shutil

import numpy as np
import pytest

from tensorflow_yolo2_amd.img_dataset import augment as A
from tensorflow_yolo2_amd.img_dataset.pascal_voc import encode_boxes, flip_label

H, W = 240, 352
# five objects of a 352 x 240 image, one per cell at 416 (S = 13) and at 96 (S = 3), classes in annotation order
OBJS = [(5.0, 8.0, 60.0, 70.0, 3), (200.0, 20.0, 340.0, 110.0, 7), (30.0, 150.0, 150.0, 236.0, 11),
        (180.0, 130.0, 260.0, 235.0, 14), (300.0, 170.0, 352.0, 240.0, 19)]

THIRD_XML = """<annotation><folder>VOC2007</folder><filename>000002.jpg</filename>
<size><width>352</width><height>240</height><depth>3</depth></size>
<object><name>car</name><difficult>0</difficult><bndbox><xmin>1</xmin><ymin>1</ymin><xmax>352</xmax><ymax>240</ymax></bndbox></object>
<object><name>cat</name><difficult>0</difficult><bndbox><xmin>30</xmin><ymin>40</ymin><xmax>120</xmax><ymax>200</ymax></bndbox></object>
<object><name>bird</name><difficult>1</difficult><bndbox><xmin>35</xmin><ymin>45</ymin><xmax>118</xmax><ymax>190</ymax></bndbox></object>
</annotation>
"""


def build_devkit(root, golden_dir, copies=1):
    """testImg2 (353 x 500, golden annotation) `copies` times, then testImg1 (352 x 240) with a hand-made annotation of
    three objects, two of which (the cat and the bird) share a cell"""
    voc = os.path.join(root, "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(voc, d), exist_ok=True)
    names = ["%06d" % (i + 1) for i in range(copies + 1)]
    for name in names[:-1]:
        shutil.copy(os.path.join(golden_dir, "testImg2.jpg"), os.path.join(voc, "JPEGImages", name + ".jpg"))
        shutil.copy(os.path.join(golden_dir, "testImg2Anno.xml"), os.path.join(voc, "Annotations", name + ".xml"))
    shutil.copy(os.path.join(golden_dir, "testImg1.jpg"), os.path.join(voc, "JPEGImages", names[-1] + ".jpg"))
    with open(os.path.join(voc, "Annotations", names[-1] + ".xml"), "w") as f:
        f.write(THIRD_XML)
    with open(os.path.join(voc, "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return root


def rows_equal_grid_cells(truth, count, grid):
    """every used row is, as float32 bits, [1:5] + the arg-max class of one occupied cell of `grid`, each cell once;
    returns the classes in list order"""
    grid32 = np.asarray(grid, np.float32)
    cells = [tuple(c) for c in np.argwhere(grid32[:, :, 0] == 1)]
    assert truth.dtype == np.float32 and truth.shape[1] == 5
    assert not truth[count:].any()
    taken = []
    for k in range(count):
        hit = [c for c in cells if np.array_equal(grid32[c][1:5].view(np.uint32), truth[k, :4].view(np.uint32))
               and int(np.argmax(grid32[c][5:])) == int(truth[k, 4])]
        assert len(hit) == 1, (k, truth[k], hit)
        taken.append(hit[0])
    assert len(set(taken)) == count
    return cells, [int(v) for v in truth[:count, 4]]


@pytest.mark.parametrize("size", (416, 96))
def test_plain_and_mirrored_rows_equal_the_grid_cells(size):
    S = size // 32
    plain = encode_boxes(OBJS, H, W, size, S)
    assert int(plain[:, :, 0].sum()) == len(OBJS)                       # one object per cell: nothing lost to a collision
    truth, count = A.encode_box_list(OBJS, A.identity_row(H, W), size, 30)
    assert truth.shape == (30, 5) and count == 5
    cells, classes = rows_equal_grid_cells(truth, count, plain)
    assert classes == [o[4] for o in OBJS] and len(cells) == 5          # annotation order
    # the identity window IS the plain path
    assert np.array_equal(A.encode_boxes_window(OBJS, A.identity_row(H, W), size, S), plain)
    # a mirrored entry, a mirrored row, and both (they cancel)
    for entry_flip, row_flip, mirrored in ((True, 0, True), (False, 1, True), (True, 1, False)):
        t2, c2 = A.encode_box_list(OBJS, A.identity_row(H, W, row_flip), size, 30, flip=entry_flip)
        rows_equal_grid_cells(t2, c2, flip_label(plain, size) if mirrored else plain)
        assert c2 == 5 and np.array_equal(t2[:, 1:], truth[:, 1:])
        assert np.array_equal(t2[:, 0], truth[:, 0]) != mirrored


def test_windowed_rows_drop_and_clamp_like_the_grid():
    size, S = 416, 13
    # a window that cuts the left 60 columns: the first object's centre leaves it (dropped), the third is clamped at x = 0
    row = np.array([60, -10, 292, 270, 0, 0.05, 1.2, 0.9], np.float64)
    for flip in (False, True):
        grid = A.encode_boxes_window(OBJS, row, size, S, 20, flip)
        truth, count = A.encode_box_list(OBJS, row, size, 30, flip)
        assert count == 4 == int(grid[:, :, 0].sum())
        _, classes = rows_equal_grid_cells(truth, count, grid)
        assert classes == [7, 11, 14, 19]
        third = truth[1]
        assert third[2] == np.float32(89.0 * (size / 292.0)) < np.float32((150.0 - 30.0) * (size / 292.0))   # clamped: narrower than the unclamped box
    # a clamp on the far side too: the window ends inside the last object
    row2 = np.array([0, 0, 330, 236, 1, 0, 1, 1], np.float64)
    grid = A.encode_boxes_window(OBJS, row2, size, S, 20, False)
    truth, count = A.encode_box_list(OBJS, row2, size, 30, False)
    assert count == 5
    rows_equal_grid_cells(truth, count, grid)
    assert truth[4, 0] == np.float32(size - 1 - ((299.0 * (size / 330.0)) + (size - 1)) / 2.0)
    # a window that holds no centre at all
    t0, c0 = A.encode_box_list(OBJS, np.array([400, 300, 50, 50, 0, 0, 1, 1], np.float64), size, 30)
    assert c0 == 0 and not t0.any()


def test_max_boxes_cuts_in_annotation_order():
    size = 416
    full, count = A.encode_box_list(OBJS, A.identity_row(H, W), size, 30)
    for T in (1, 3, 5):
        t, c = A.encode_box_list(OBJS, A.identity_row(H, W), size, T)
        assert t.shape == (T, 5) and c == min(T, 5) and np.array_equal(t, full[:T])
    # the cut counts KEPT objects: with the first one dropped by the window, T = 1 holds the second
    row = np.array([60, -10, 292, 270, 0, 0, 1, 1], np.float64)
    t, c = A.encode_box_list(OBJS, row, size, 1)
    assert c == 1 and t[0, 4] == 7
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            A.encode_box_list(OBJS, A.identity_row(H, W), size, bad)


@pytest.mark.parametrize("mode", ("plain", "flipped", "augment"))
def test_host_batcher_returns_the_box_list(tmp_path, golden_dir, mode):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    kw = dict(batch_size=2, devkit_path=kit, image_size=416, flipped=(mode == "flipped"), seed=5, cache_images=False)
    if mode == "augment":
        kw["augment"] = A.Augment()
    ds = pascal_voc("trainval", max_boxes=6, **kw)
    pair = pascal_voc("trainval", **kw)
    seen_collision = False
    for _ in range(3):
        images, labels, truth, ntruth = ds.get_u8()
        im2, lab2 = pair.get_u8()                              # max_boxes=None: the pair, and the same batch
        assert np.array_equal(images, im2) and np.array_equal(labels, lab2)
        assert truth.shape == (2, 6, 5) and truth.dtype == np.float32 and ntruth.shape == (2,) and ntruth.dtype == np.int32
        for b in range(2):
            n = int(ntruth[b])
            assert not truth[b, n:].any()
            cells = int((labels[b, :, :, 0] == 1).sum())
            assert n >= cells
            seen_collision |= n > cells
            # every occupied cell is some row of the list, bit for bit
            for c in np.argwhere(labels[b, :, :, 0] == 1):
                cell = labels[b, c[0], c[1]]
                assert any(np.array_equal(cell[1:5].view(np.uint32), truth[b, k, :4].view(np.uint32))
                           and int(np.argmax(cell[5:])) == int(truth[b, k, 4]) for k in range(n))
    if mode != "augment":
        assert seen_collision                                   # testImg1's cat and bird share a cell: the list keeps both
    f = pascal_voc("trainval", max_boxes=6, **kw).get()
    assert len(f) == 4 and f[0].dtype == np.float32 and f[2].shape == (2, 6, 5)
    with pytest.raises(ValueError):
        pascal_voc("trainval", max_boxes=0, **kw)


def test_testimg1_list_holds_three_objects_where_the_grid_holds_fewer(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import parse_annotation
    objs, shape = parse_annotation(THIRD_XML)
    assert shape == (240, 352) and len(objs) == 3
    grid = encode_boxes(objs, shape[0], shape[1], 416, 13)
    truth, count = A.encode_box_list(objs, A.identity_row(*shape), 416, 30)
    assert count == 3 > int(grid[:, :, 0].sum())
    assert [int(v) for v in truth[:3, 4]] == [6, 7, 2]          # car, cat, bird in annotation order


def test_train_script_flags_need_box_labels(capsys):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as T
    for extra in (["--area-weight"], ["--prior-images", "12800"], ["--max-boxes", "10"]):
        with pytest.raises(SystemExit):
            T.parse_args(["--devkit", "x"] + extra)
        assert "--box-labels" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        T.parse_args(["--devkit", "x", "--box-labels", "--max-boxes", "0"])
    a = T.parse_args(["--devkit", "x"])
    assert (a.box_labels, a.max_boxes, a.area_weight, a.prior_images) == (False, 30, False, 0)
    a = T.parse_args(["--devkit", "x", "--box-labels", "--area-weight", "--prior-images", "12800", "--max-boxes", "50"])
    assert (a.box_labels, a.max_boxes, a.area_weight, a.prior_images) == (True, 50, True, 12800)
