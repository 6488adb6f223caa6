"""Darknet's dataset files on the host (utils/darknet_data.py): the .data grammar and its refusals, the label path rule,
the label reader's refusals, label rows -> box table -> box list to one float32 ulp, the round trip of a converted
devkit, negatives, and the COCO training entries.  No GPU."""
import json
import os

import numpy as np
import pytest

from test_box_list_host import build_devkit
from tensorflow_yolo2_amd.img_dataset import augment as A
from tensorflow_yolo2_amd.utils import darknet_data as DD


def _write(path, text):
    with open(str(path), "w") as f:
        f.write(text)
    return str(path)


def test_data_grammar_comments_duplicates_and_refusals(tmp_path):
    p = _write(tmp_path / "voc.data",
               "# a comment\n; another\n\n  classes = 3 \ntrain=/x/train.txt\nvalid = lists/val.txt\nnames=data/my.names\n"
               "backup = backup/\nclasses=5\nresults=results\n")
    d = DD.read_data(p)
    assert d.classes == 5                                               # the later duplicate wins
    assert (d.train, d.valid, d.names, d.backup, d.results) == ("/x/train.txt", "lists/val.txt", "data/my.names",
                                                                "backup/", "results")       # kept as written
    assert d.eval == "voc" and d.path == p
    with pytest.raises(AttributeError):
        d.classes = 2                                                   # immutable
    d = DD.read_data(_write(tmp_path / "coco.data", "classes=80\neval=coco\n"))
    assert d.eval == "coco" and d.train is None and d.backup is None
    for text, line, word in (("classes=3\ntop=5\n", 2, "top"),                   # a key Darknet has and this tree not
                             ("classes=three\n", 1, "classes"),
                             ("train=a.txt\nclasses=0\n", 2, "classes"),
                             ("classes=3\n\neval=imagenet\n", 3, "eval"),
                             ("classes=3\n# c\njust words\n", 3, "just words"),
                             ("classes=3\ntrain=\n", 2, "train"),
                             ("train=a.txt\n", 1, "classes")):
        p = _write(tmp_path / "bad.data", text)
        with pytest.raises(ValueError) as e:
            DD.read_data(p)
        assert str(e.value).startswith("%s:%d: " % (p, line)) and word in str(e.value), (text, str(e.value))


def test_label_path_rule():
    assert DD.label_path("/d/coco/images/train2014/a.jpg") == "/d/coco/labels/train2014/a.txt"
    assert DD.label_path("/d/VOCdevkit/VOC2007/JPEGImages/000001.jpg") == "/d/VOCdevkit/VOC2007/labels/000001.txt"
    assert DD.label_path("/d/images/x/images/b.jpg") == "/d/labels/x/images/b.txt"            # only the first
    assert DD.label_path("/d/raw/b.png") == "/d/labels/b.txt"
    assert DD.label_path("/d/images/b.JPEG") == "/d/labels/b.txt"
    assert DD.label_path("/d/pics/b.JPG") == "/d/pics/b.txt"
    # every rule is applied once to the result of the one before: `images`, then `JPEGImages`, then `raw`
    assert DD.label_path("/raw/JPEGImages/c.jpg") == "/labels/labels/c.txt"
    assert DD.label_path("/d/images/raw/images/c.jpg") == "/d/labels/labels/images/c.txt"
    with pytest.raises(ValueError, match="pics/b.bmp"):
        DD.label_path("/d/pics/b.bmp")


def test_read_labels_and_its_refusals(tmp_path):
    p = _write(tmp_path / "e.txt", "")
    assert DD.read_labels(p, 3) == []                                   # an image without objects
    p = _write(tmp_path / "ok.txt", "0 0.5 0.5 0.25 0.125\n\n2 1e-1 .9 0.2 0.1\n")
    assert DD.read_labels(p, 3) == [(0, 0.5, 0.5, 0.25, 0.125), (2, 0.1, 0.9, 0.2, 0.1)]
    for text, line, word in (("0 .5 .5 .1 .1\n3 .5 .5 .1 .1\n", 2, "class 3"),
                             ("-1 .5 .5 .1 .1\n", 1, "class -1"),
                             ("0 .5 .5 .1\n", 1, "4 values"),
                             ("0 .5 nan .1 .1\n", 1, "cy=nan"),
                             ("0 .5 .5 inf .1\n", 1, "w=inf"),
                             ("0 .5 .5 0 .1\n", 1, "w=0"),
                             ("0 .5 .5 .1 -0.2\n", 1, "h=-0.2"),
                             ("0 .5 x .1 .1\n", 1, "cy=x"),
                             ("1.5 .5 .5 .1 .1\n", 1, "class 1.5")):
        p = _write(tmp_path / "bad.txt", text)
        with pytest.raises(ValueError) as e:
            DD.read_labels(p, 3)
        assert str(e.value).startswith("%s:%d: " % (p, line)) and word in str(e.value), (text, str(e.value))
    with pytest.raises(ValueError, match="images/q.jpg"):
        DD.read_labels(str(tmp_path / "missing.txt"), 3, image="/d/images/q.jpg")


def _ulp_apart(got, want):
    """distance in float32 ulps of two float32 arrays of one sign"""
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("size", (96, 416, 608))
def test_label_rows_through_the_box_table_come_back_to_one_ulp(size):
    """to_pixel_boxes then encode_box_list under identity_row: cx * size, cy * size, w * size, h * size to one float32 ulp
    (double arithmetic and one cast: one ulp of the cast is the whole budget).  The boxes lie inside the image and stop
    short of its right and bottom edge by construction: the clamp to size - 1 would move those"""
    rng = np.random.default_rng(5)
    for (H, W) in ((375, 500), (480, 353), (240, 352), (1, 7)):
        rows = []
        for k in range(60):
            w, h = rng.uniform(0.01, 0.6), rng.uniform(0.01, 0.6)
            # xmax * size < size - 1  <=>  cx + w / 2 < 1 - 1 / size; a margin of 2 / size keeps rounding away
            cx = rng.uniform(w / 2 + 1e-3, 1 - w / 2 - 2.0 / size)
            cy = rng.uniform(h / 2 + 1e-3, 1 - h / 2 - 2.0 / size)
            rows.append((int(rng.integers(0, 5)), cx, cy, w, h))
        objs = DD.to_pixel_boxes(rows, H, W)
        for (xmin, ymin, xmax, ymax, _c), (_c2, cx, cy, w, h) in zip(objs, rows):
            assert xmin == (cx - w / 2) * W + 1 and ymax == (cy + h / 2) * H + 1       # each operation on its own
        truth, count = A.encode_box_list(objs, A.identity_row(H, W), size, 64)
        assert count == 60
        want = np.array([[cx * size, cy * size, w * size, h * size] for (_c, cx, cy, w, h) in rows]).astype(np.float32)
        worst = int(_ulp_apart(truth[:60, :4], want).max())
        print("size %d, image %d x %d: at most %d ulp" % (size, W, H, worst))
        assert worst <= 1
        assert truth[:60, 4].tolist() == [float(r[0]) for r in rows]


def _devkit_as_list(kit, root):
    """the devkit's images copied under root/images with label files through write_labels -> (list path, entries)"""
    import shutil
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import read_image_set
    _index, entries = read_image_set(os.path.join(kit, "VOC2007"), "trainval")
    os.makedirs(os.path.join(root, "images"))
    paths = []
    for e in entries:
        dst = os.path.join(root, "images", os.path.basename(e['imname']))
        shutil.copy(e['imname'], dst)
        DD.write_labels(DD.label_path(dst), DD.from_pixel_boxes(e['objs'], *e['shape']))
        paths.append(dst)
    return _write(os.path.join(root, "train.txt"), "\n".join(paths) + "\n"), entries


def test_a_converted_devkit_round_trips_and_keeps_negatives(tmp_path, golden_dir):
    kit = build_devkit(str(tmp_path / "VOCdevkit"), golden_dir, copies=1)
    lst, voc = _devkit_as_list(kit, str(tmp_path / "dk"))
    assert DD.read_list(lst) == [os.path.join(str(tmp_path / "dk"), "images", n) for n in ("000001.jpg", "000002.jpg")]
    for e in voc:
        p = DD.label_path(os.path.join(str(tmp_path / "dk"), "images", os.path.basename(e['imname'])))
        rows = DD.from_pixel_boxes(e['objs'], *e['shape'])
        assert DD.read_labels(p, 20) == rows                            # write_labels -> read_labels: the same float64
        back = np.asarray(DD.to_pixel_boxes(rows, *e['shape']))
        np.testing.assert_allclose(back, np.asarray(e['objs'], np.float64), rtol=0, atol=1e-9)
    # an image with an empty label file is an entry with no object, and stays in the list
    import shutil
    neg = os.path.join(str(tmp_path / "dk"), "images", "neg.jpg")
    shutil.copy(os.path.join(golden_dir, "testImg1.jpg"), neg)
    DD.write_labels(DD.label_path(neg), [])
    with open(lst, "a") as f:
        f.write("\n" + neg + "\n")
    entries = DD.image_entries(lst, 20)
    assert [len(e['objs']) for e in entries] == [len(voc[0]['objs']), 3, 0]
    assert entries[2]['shape'] == (240, 352) and entries[2]['difficult'] == [] and entries[1]['difficult'] == [0, 0, 0]
    assert [e['shape'] for e in entries[:2]] == [e['shape'] for e in voc]
    # a listed image that is not there names list:line; a missing label file names its image
    bad = _write(tmp_path / "bad.txt", lst.replace("train.txt", "images/000001.jpg") + "\n\n/nowhere/images/x.jpg\n")
    with pytest.raises(ValueError, match=r"bad\.txt:3: .*x\.jpg"):
        DD.read_list(bad)
    os.remove(DD.label_path(neg))
    with pytest.raises(ValueError, match="neg.jpg"):
        DD.image_entries(lst, 20)
    with pytest.raises(ValueError, match=r"outside 0\.\.2"):           # the devkit's classes do not fit classes=3
        DD.image_entries(_write(tmp_path / "two.txt", DD.read_list(lst)[1] + "\n"), 3)


def test_image_id_of_a_coco_file_name():
    assert DD.image_id_of("/d/val2014/COCO_val2014_000000000139.jpg") == 139
    assert DD.image_id_of("000042.png") == 42
    with pytest.raises(ValueError):
        DD.image_id_of("/d/cat.jpg")


def test_coco_training_entries(tmp_path, golden_dir):
    from tensorflow_yolo2_amd.img_dataset.device_coco import train_entries
    from tensorflow_yolo2_amd.utils import coco_eval
    src = os.path.join(golden_dir, "coco", "instances_tiny.json")
    data = json.load(open(src))
    # two zero-extent annotations beside the fixture's crowd one
    data["annotations"] += [{"id": 990, "image_id": 19, "category_id": 3, "bbox": [10.0, 10.0, 0.0, 30.0], "area": 0.0,
                             "iscrowd": 0},
                            {"id": 991, "image_id": 19, "category_id": 1, "bbox": [10.0, 10.0, 20.0, -1.0], "area": 0.0,
                             "iscrowd": 0},
                            {"id": 992, "image_id": 19, "category_id": 17, "bbox": [1.5, 2.0, 20.0, 30.25], "area": 600.0,
                             "iscrowd": 0}]
    p = _write(tmp_path / "instances.json", json.dumps(data))
    for path, last in ((src, []), (p, [(2.5, 3.0, 22.5, 33.25, 2)])):
        ds = coco_eval.read_instances(path)
        assert ds["categories"] == [1, 3, 17]                           # person, car, cat -> 0, 1, 2
        entries = train_entries(ds["images"], "/img")
        assert [e['id'] for e in entries] == [7, 19, 42]                # ascending image id
        assert [e['imname'] for e in entries] == ["/img/testImg1.jpg", "/img/testImg1.jpg", "/img/testImg2.jpg"]
        assert [e['shape'] for e in entries] == [(240, 352), (240, 352), (500, 353)]
        assert entries[0]['objs'] == [(41.0, 51.0, 191.0, 151.0, 1), (201.0, 101.0, 301.5, 221.0, 2),
                                      (6.0, 6.0, 66.0, 206.0, 0)]
        assert entries[1]['objs'] == last                               # zero and negative extents are absent
        # image 42: the crowd annotation (cat, 904) is absent; file order otherwise
        assert entries[2]['objs'] == [(31.5, 61.25, 231.5, 441.75, 0), (201.0, 301.0, 321.0, 391.0, 1),
                                      (301.0, 21.0, 321.5, 51.0, 0)]
        assert all(e['difficult'] == [0] * len(e['objs']) for e in entries)
