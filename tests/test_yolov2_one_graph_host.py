"""The snapshot front of both YOLOv2 topologies (yolo2_nets/net_utils.py) and the model flags that pascal_eval_yolov2.py
and pascal_detect_yolov2.py share (pascal/yolov2_model_flags.py): no GPU, a temporary directory of empty files."""
import os

import pytest


def _touch(directory, names):
    os.makedirs(directory, exist_ok=True)
    for name in names:
        open(os.path.join(directory, name), "wb").close()


@pytest.mark.parametrize("topology,ext,lister", [("paper", ".npz", "get_ordered_yolov2_ckpts"),
                                                 ("darknet", ".weights", "get_ordered_darknet_ckpts")])
def test_snapshots_are_ordered_by_iteration_number_not_by_name(tmp_path, topology, ext, lister):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    d = str(tmp_path / "ckpt")
    assert getattr(net_utils, lister)(d) == [] and net_utils.latest_yolov2_snapshot(d, topology) is None
    # files that are no snapshot of this topology's: another prefix, another tag, no number, a longer extension
    _touch(d, ["train_iter_10" + ext, "train_iter_9" + ext, "train_iter_100" + ext, "train_iter_2" + ext,
               "test_iter_500" + ext, "train_epoch_700" + ext, "train_iter_x" + ext, "train_iter_800" + ext + ".tmp"])
    want = [os.path.join(d, "train_iter_%d%s" % (i, ext)) for i in (2, 9, 10, 100)]
    assert getattr(net_utils, lister)(d) == want
    assert net_utils.latest_yolov2_snapshot(d, topology) == want[-1]


def test_a_directory_of_the_other_topology_is_refused_in_both_directions(tmp_path):
    from tensorflow_yolo2_amd.yolo2_nets import net_utils
    paper, darknet = str(tmp_path / "paper"), str(tmp_path / "darknet")
    _touch(paper, ["train_iter_3.npz", "train_iter_20.npz"])
    _touch(darknet, ["train_iter_7.weights", "train_iter_11.weights"])
    with pytest.raises(ValueError) as e:
        net_utils.latest_yolov2_snapshot(paper, "darknet")
    assert str(e.value) == ("--ckpt-dir %s holds snapshots of the paper topology (train_iter_20.npz); this run trains the "
                            "darknet topology, whose snapshots are .weights files" % paper)
    with pytest.raises(ValueError) as e:
        net_utils.latest_yolov2_snapshot(darknet, "paper")
    assert str(e.value) == ("--ckpt-dir %s holds snapshots of the darknet topology (train_iter_11.weights); this run trains "
                            "the paper topology, whose snapshots are .npz files" % darknet)
    # a directory that holds both is refused as well: the other topology's files are looked for first
    _touch(paper, ["train_iter_1.weights"])
    with pytest.raises(ValueError):
        net_utils.latest_yolov2_snapshot(paper, "paper")


SCRIPTS = [("pascal_eval_yolov2", ["--devkit", "kit"]), ("pascal_detect_yolov2", ["--images", "a.jpg"])]


@pytest.mark.parametrize("script,base", SCRIPTS)
@pytest.mark.parametrize("flags,message", [
    (["--darknet-weights", "m.weights", "--weights", "s.npz"], "--darknet-weights goes with neither --weights nor --ckpt-dir"),
    (["--darknet-weights", "m.weights", "--ckpt-dir", "d"], "--darknet-weights goes with neither --weights nor --ckpt-dir"),
    (["--size", "100"], "--size 100: the detector head needs a positive multiple of 32 (S = size / 32)"),
    (["--size", "0"], "--size 0: the detector head needs a positive multiple of 32 (S = size / 32)"),
    (["--size", "672"], "--size 672: more than 2048 candidates per image"),
])
def test_shared_model_flags_are_checked_through_both_scripts(capsys, script, base, flags, message):
    import importlib
    mod = importlib.import_module("tensorflow_yolo2_amd.pascal." + script)
    with pytest.raises(SystemExit) as e:
        mod.parse_args(base + flags)
    assert e.value.code == 2
    assert capsys.readouterr().err.rstrip().endswith("error: " + message)


@pytest.mark.parametrize("script,base", SCRIPTS)
def test_shared_model_flags_keep_their_defaults_and_limits(script, base):
    import importlib
    mod = importlib.import_module("tensorflow_yolo2_amd.pascal." + script)
    a = mod.parse_args(base)
    assert (a.size, a.dtype, a.weights, a.ckpt_dir, a.darknet_weights, a.width_div, a.keep_grids) == \
        (416, "f16", None, None, None, 1, False)
    assert a.batch == (32 if script == "pascal_eval_yolov2" else 1)
    # 20 x 20 cells x 5 anchors = 2000 candidates pass, 21 x 21 x 5 = 2205 do not (the case above)
    assert mod.parse_args(base + ["--size", "640", "--darknet-weights", "m.weights"]).darknet_weights == "m.weights"
