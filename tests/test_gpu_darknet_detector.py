"""Darknet's detector command over Darknet's own files (darknet/detector.py) and COCO training (coco/coco_train_yolov2.py)
on the GPU: a 3-class cfg at narrow widths (tests/golden/cfg/narrow-tiny.cfg), a list of six small images with label
files, batch 4, size 96."""
import json
import os

import numpy as np
import pytest

from test_gpu_device_darknet import make_list

gpu = pytest.mark.gpu
FLAGS = ["--batch", "4", "--size", "96", "--dtype", "f32"]


def data_file(root, lst, **keys):
    """a .data file of 3 classes over the list, with names, backup and results under root"""
    with open(os.path.join(root, "three.names"), "w") as f:
        f.write("ball\ncone\ncube\n")
    entries = dict(classes="3", train=lst, valid=lst, names=os.path.join(root, "three.names"),
                   backup=os.path.join(root, "backup"), results=os.path.join(root, "results"))
    entries.update(keys)
    path = os.path.join(root, "three_%d.data" % len(os.listdir(root)))
    with open(path, "w") as f:
        f.write("# a data set of three classes\n" + "".join("%s = %s\n" % kv for kv in entries.items() if kv[1] is not None))
    return path


@gpu
def test_detector_train_valid_map_and_anchors(tmp_path, tmp_path_factory, golden_dir, capsys):
    from test_gpu_darknet_cfg import weights_file
    from tensorflow_yolo2_amd.darknet import detector
    from tensorflow_yolo2_amd.utils import darknet_weights as DW
    root = str(tmp_path)
    lst = make_list(root, golden_dir)
    cfg = os.path.join(golden_dir, "cfg", "narrow-tiny.cfg")
    data = data_file(root, lst)
    train = FLAGS + ["--single-scale", "--region-stats"]
    first = detector.main(["train", data, cfg, "--iters", "3"] + train)
    out = capsys.readouterr().out
    assert "topology tiny, 3 classes, 5 anchors, size 96, batch 4, multi-scale off" in out
    assert np.isfinite(np.array(first["losses"])).all() and len(first["losses"]) == 3 and first["first_iter"] == 1
    imdb = first["imdb"]
    assert imdb.draw and imdb.max_boxes == 30 and imdb.augment is not None and imdb.classes == ("ball", "cone", "cube")
    assert np.isfinite(np.array(first["region_stats"])).all()
    snap = os.path.join(root, "backup", "train_iter_3.weights")
    assert os.path.exists(snap) and DW.read(snap)[3] == 12           # seen = 3 iterations of 4 images
    second = detector.main(["train", data, cfg, "--iters", "2"] + train)      # resumes from backup=
    assert "Restorining model snapshots from " + snap in capsys.readouterr().out
    assert second["first_iter"] == 4 and second["last_iter"] == 5 and np.isfinite(np.array(second["losses"])).all()
    assert os.path.exists(os.path.join(root, "backup", "train_iter_5.weights"))
    # [weights]: a whole model by its float count (no backup= here: nothing to resume from, nothing written)
    whole, rec, _layers = weights_file(tmp_path_factory, golden_dir, "narrow-tiny.cfg", seed=4, seen=8)
    third = detector.main(["train", data_file(root, lst, backup=None), cfg, whole, "--iters", "1"] + train)
    assert "Model restored from Darknet weight file " + whole in capsys.readouterr().out and len(third["losses"]) == 1
    # valid: one results file per class, Darknet's "%f" rows; no label file is read
    res = detector.main(["valid", data, cfg, snap, "--thresh", "0.001"] + FLAGS)
    files = res["results_files"]
    assert [os.path.basename(p) for p in files] == ["comp4_det_test_%s.txt" % c for c in ("ball", "cone", "cube")]
    assert all(os.path.dirname(p) == os.path.join(root, "results") and os.path.exists(p) for p in files)
    lines = [ln.split() for p in files for ln in open(p).read().splitlines()]
    assert len(lines) == len(res["rows"]["score"]) > 0 and all(len(ln) == 6 and ln[0].startswith("im") for ln in lines)
    assert res["imdb"].counts.cpu().numpy().sum() == 0
    # eval=coco: the JSON, image ids from the digits of the file names
    res = detector.main(["valid", data_file(root, lst, eval="coco"), cfg, snap, "--thresh", "0.001"] + FLAGS)
    rows = json.load(open(res["results_files"][0]))
    assert os.path.basename(res["results_files"][0]) == "coco_results.json" and len(rows) == len(res["rows"]["score"]) > 0
    assert set(r["image_id"] for r in rows) <= set(range(6)) and set(r["category_id"] for r in rows) <= {1, 2, 3}
    assert all(len(r["bbox"]) == 4 and np.isfinite(r["bbox"]).all() and 0 <= r["score"] <= 1 for r in rows)
    # map: one finite AP per class over the list's own label files
    capsys.readouterr()
    for metric in ("07", "10"):
        res = detector.main(["map", data, cfg, snap, "--metric", metric, "--thresh", "0.001"] + FLAGS)
        assert sorted(res["aps"]) == [0, 1, 2] and all(np.isfinite(v) and 0 <= v <= 1 for v in res["aps"].values())
        assert np.isfinite(res["mAP"]) and len(res["imdb"].entries) == 6
        out = capsys.readouterr().out
        assert "AP for ball = " in out and "AP for cube = " in out and "Mean AP = " in out
    # anchors: two pairs as a cfg line
    res = detector.main(["anchors", data, "--num", "2", "--size", "96"])
    out = capsys.readouterr().out
    (line,) = [ln for ln in out.splitlines() if ln.startswith("anchors = ")]
    assert len(line[len("anchors = "):].replace(" ", "").split(",")) == 4 and "mean_shape_iou = " in out
    assert res["anchors"].shape == (2, 2) and 0 < res["mean_shape_iou"] <= 1 and res["boxes"] == 17


def test_detector_refuses_files_that_disagree(tmp_path, golden_dir, capsys):
    from tensorflow_yolo2_amd.darknet import detector
    root = str(tmp_path)
    lst = make_list(root, golden_dir)
    cfg = os.path.join(golden_dir, "cfg", "narrow-tiny.cfg")
    with open(os.path.join(root, "two.names"), "w") as f:
        f.write("ball\ncone\n")
    cases = ((data_file(root, lst, names=os.path.join(root, "two.names")), ("two.names", ".data", "2 names")),
             (data_file(root, lst, classes="4", names=None), ("narrow-tiny.cfg", ".data", "classes=4", "classes=3")),
             (data_file(root, lst, train=None), ("train=",)))
    for data, words in cases:
        with pytest.raises(SystemExit):
            detector.main(["train", data, cfg, "--iters", "1"] + FLAGS)
        err = capsys.readouterr().err
        assert all(w in err for w in words), err
    with pytest.raises(SystemExit):                                  # a .data file with a key this tree does not read
        with open(os.path.join(root, "odd.data"), "w") as f:
            f.write("classes=3\ntop=5\n")
        detector.main(["anchors", os.path.join(root, "odd.data"), "--num", "2", "--size", "96"])
    assert "odd.data:2: " in capsys.readouterr().err
    with pytest.raises(SystemExit):
        detector.main(["valid", data_file(root, lst), cfg])          # no weights
    assert ".weights" in capsys.readouterr().err


@gpu
def test_coco_training_runs_on_the_tiny_instances_file(tmp_path, golden_dir, capsys):
    from tensorflow_yolo2_amd.coco import coco_train_yolov2
    cfg = os.path.join(golden_dir, "cfg", "narrow-tiny.cfg")
    ckpt = str(tmp_path / "backup")
    res = coco_train_yolov2.main(["--annotations", os.path.join(golden_dir, "coco", "instances_tiny.json"), "--images",
                                  golden_dir, "--cfg", cfg, "--ckpt-dir", ckpt, "--iters", "2", "--max-boxes", "2",
                                  "--single-scale"] + FLAGS)
    assert len(res["losses"]) == 2 and np.isfinite(np.array(res["losses"])).all()
    imdb = res["imdb"]
    assert imdb.draw and imdb.max_boxes == 2 and imdb.num_class == 3 and imdb.image_ids == [7, 19, 42]
    assert os.path.exists(os.path.join(ckpt, "train_iter_2.weights"))
    with pytest.raises(SystemExit):                                  # 20 classes against 3 categories
        coco_train_yolov2.main(["--annotations", os.path.join(golden_dir, "coco", "instances_tiny.json"), "--images",
                                golden_dir, "--cfg", os.path.join(golden_dir, "cfg", "narrow-tiny-voc.cfg"), "--iters", "1"])
    assert "classes=20" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        coco_train_yolov2.main(["--cfg", cfg, "--iters", "1"])
    assert "--annotations" in capsys.readouterr().err
