"""Host-side tests of the "tiny" topology (tiny-yolo-voc.cfg): the file's layer list and float count, the zero padding of
its two narrow layers on import and its removal on export, which Darknet graph a `.weights` file holds, the snapshot
front, and the flags of the three callers.  No GPU."""
import os

import numpy as np
import pytest

from tensorflow_yolo2_amd.utils import darknet_weights as DW
from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2

EPS = yolov2.DARKNET_BN_EPS


def _random_layers(file_layers, seed):
    rng = np.random.default_rng(seed)
    out = []
    for (k, c, n, bn) in file_layers:
        d = {"biases": rng.normal(0, 0.2, n).astype(np.float32)}
        if bn:
            d.update(scales=rng.uniform(0.8, 1.2, n).astype(np.float32), rolling_mean=rng.normal(0, 0.2, n).astype(np.float32),
                     rolling_variance=rng.uniform(0.5, 2.0, n).astype(np.float32))
        d["weights"] = rng.normal(0, 0.1, (n, c, k, k)).astype(np.float32)
        out.append(d)
    return out


def test_layer_list_and_float_count():
    layers = DW.yolov2_tiny_voc_layers()
    assert len(layers) == 9 and layers[0] == (3, 3, 16, True) and layers[1] == (3, 16, 32, True)
    assert layers[8] == (1, 1024, 125, False) and all(l[0] == 3 and l[3] for l in layers[:8])
    assert sum(DW.layer_floats(l) for l in layers) == 15867885
    assert 16 + 4 * 15867885 == 63471556                              # the published tiny-yolo-voc.weights
    assert net_utils.darknet_graph_floats("tiny", 20, 5) == 15867885
    assert net_utils._file_layers("tiny", yolov2.yolov2_tiny_specs(20, 5, 1)) == layers
    assert net_utils._file_layers("darknet", yolov2.yolov2_darknet_specs(20, 5, 1)) == DW.yolov2_voc_layers()
    assert DW.yolov2_tiny_voc_layers(3, 2)[8] == (1, 1024, 16, False)


def test_specs_keep_the_two_narrow_layers_under_the_width_divisor():
    stem, head = yolov2.yolov2_tiny_specs(20, 5, 1)
    assert stem == [(3, 3, 32, 1), (3, 32, 32, 1), (3, 32, 64, 1), (3, 64, 128, 1), (3, 128, 256, 1), (3, 256, 512, 0)]
    assert head == [(3, 512, 1024, 0), (3, 1024, 1024, 0), (1, 1024, 125, 0)]
    stem8, head8 = yolov2.yolov2_tiny_specs(3, 5, 8)
    assert stem8[:2] == stem[:2] and stem8[5] == (3, 32, 64, 0) and head8 == [(3, 64, 128, 0), (3, 128, 128, 0), (1, 128, 40, 0)]
    files8 = net_utils._file_layers("tiny", (stem8, head8))
    assert files8[0] == (3, 3, 16, True) and files8[1] == (3, 16, 32, True) and files8[2] == (3, 32, 32, True)
    topo = yolov2._TOPOLOGY["tiny"]
    assert "tiny" in yolov2.TOPOLOGIES and topo.heights == (32, 1) and topo.concat is None and topo.cf_stack is None
    assert topo.slopes == (None, [0.1, 0.1, 1.0]) and topo.train_options[1]["core_layers"] == 2
    assert topo.bn_eps == 1e-6 and topo.darknet_input and topo.anchors == yolov2.ANCHORS_TINY_VOC
    assert yolov2.ANCHORS_TINY_VOC == ((1.08, 1.19), (3.42, 4.41), (6.63, 11.38), (9.42, 5.11), (16.62, 10.52))
    with pytest.raises(ValueError):
        yolov2._topology("small")


def _import(layers, specs):
    """what net_utils' loader does per layer, without a device: file entries -> the stacks' layer dicts"""
    flat = [s for spec in specs for s in spec]
    return [DW.pad_layer_params(DW.to_layer_params(d, k, EPS), ci, co) for d, (k, ci, co, _p) in zip(layers, flat)]


def _export(params, file_layers):
    return [DW.from_layer_params(DW.strip_layer_params(p, c, n), k, bn, EPS) for p, (k, c, n, bn) in zip(params, file_layers)]


def test_pad_on_import_and_strip_on_export_return_the_bytes(tmp_path):
    specs = yolov2.yolov2_tiny_specs(3, 5, 8)
    file_layers = net_utils._file_layers("tiny", specs)
    layers = _random_layers(file_layers, 1)
    path = str(tmp_path / "tiny.weights")
    DW.write(path, layers, 64000)
    read, used = DW.split(DW.read(path)[4], file_layers)
    assert used == net_utils.darknet_graph_floats("tiny", 3, 5, 8)
    params = _import(read, specs)
    p0, p1 = params[0], params[1]
    assert p0["W"].shape == (3, 3, 3, 32) and p1["W"].shape == (3, 3, 32, 32)
    np.testing.assert_array_equal(p0["W"][..., :16], layers[0]["weights"].transpose(2, 3, 1, 0))
    np.testing.assert_array_equal(p1["W"][:, :, :16], layers[1]["weights"].transpose(2, 3, 1, 0))
    assert not p0["W"][..., 16:].any() and not p1["W"][:, :, 16:].any()
    for key, fill in (("b", 0), ("gamma", 1), ("beta", 0), ("moving_mean", 0), ("moving_var", 1)):
        assert (p0[key][16:] == fill).all() and p0[key].shape == (32,), key
    np.testing.assert_array_equal(p0["gamma"][:16], layers[0]["scales"])
    back = str(tmp_path / "back.weights")
    DW.write(back, _export(params, file_layers), 64000)
    assert open(back, "rb").read() == open(path, "rb").read()
    # layers of the file's own width pass through untouched
    assert DW.pad_layer_params(params[2], 32, 32) is params[2] and DW.strip_layer_params(params[2], 32, 32) is params[2]
    with pytest.raises(ValueError):
        DW.pad_layer_params(params[2], 16, 32)
    with pytest.raises(ValueError):
        DW.strip_layer_params(params[2], 64, 32)


@pytest.mark.parametrize("layer,key,index", [(0, "W", (1, 1, 2, 20)), (0, "b", (17,)), (0, "beta", (31,)),
                                             (0, "moving_mean", (16,)), (1, "W", (0, 2, 16, 5))])
def test_export_refuses_a_non_zero_padded_entry(layer, key, index):
    specs = yolov2.yolov2_tiny_specs(3, 5, 8)
    file_layers = net_utils._file_layers("tiny", specs)
    params = _import(_random_layers(file_layers, 2), specs)
    _export(params, file_layers)
    params[layer][key][index] = 1e-30
    with pytest.raises(ValueError) as e:
        _export(params, file_layers)
    assert "padded entries" in str(e.value) and key in str(e.value)


def test_padded_variance_and_scale_may_move():
    """training moves the padded filters' moving variance (their batch variance is 0); it scales an exact zero"""
    specs = yolov2.yolov2_tiny_specs(3, 5, 8)
    file_layers = net_utils._file_layers("tiny", specs)
    params = _import(_random_layers(file_layers, 3), specs)
    want = _export(params, file_layers)
    params[0]["moving_var"][16:] = 0.96
    got = _export(params, file_layers)
    for a, b in zip(got, want):
        for key in a:
            assert a[key].tobytes() == b[key].tobytes()


def test_darknet_file_topology(tmp_path):
    paths = {}
    for t in yolov2.DARKNET_FILE_TOPOLOGIES:
        file_layers = net_utils._file_layers(t, yolov2._TOPOLOGY[t].specs(3, 5, 8))
        paths[t] = str(tmp_path / (t + ".weights"))
        DW.write(paths[t], _random_layers(file_layers, 4), 7)
        assert net_utils.darknet_file_topology(paths[t], 3, 5, 8) == t
    n_full, n_tiny = (net_utils.darknet_graph_floats(t, 3, 5, 8) for t in ("darknet", "tiny"))
    assert n_full != n_tiny
    with pytest.raises(ValueError) as e:
        net_utils.darknet_file_topology(paths["tiny"], 4, 5, 8)
    msg = str(e.value)
    assert str(net_utils.darknet_graph_floats("darknet", 4, 5, 8)) in msg and "\"darknet\"" in msg
    assert str(net_utils.darknet_graph_floats("tiny", 4, 5, 8)) in msg and "\"tiny\"" in msg
    assert paths["tiny"] in msg and str(n_tiny) in msg


def test_snapshot_front_treats_tiny_as_a_weights_topology(tmp_path):
    class Model:
        def __init__(self, topology):
            self.topology = topology
    assert net_utils._is_darknet(Model("tiny")) and net_utils._is_darknet(Model("darknet"))
    assert not net_utils._is_darknet(Model("paper")) and not net_utils._is_darknet(object())
    assert net_utils._SNAPSHOT_EXT == {"paper": ".npz", "darknet": ".weights", "tiny": ".weights"}
    d = str(tmp_path / "weights")
    os.makedirs(d)
    assert net_utils.latest_yolov2_snapshot(d, "tiny") is None
    for i in (3, 20, 100):
        open(os.path.join(d, "train_iter_%d.weights" % i), "wb").close()
    # the two Darknet graphs share the format: the listing cannot tell them apart, the loader does (by the float count)
    assert net_utils.latest_yolov2_snapshot(d, "tiny") == os.path.join(d, "train_iter_100.weights")
    assert net_utils.latest_yolov2_snapshot(d, "darknet") == os.path.join(d, "train_iter_100.weights")
    with pytest.raises(ValueError) as e:
        net_utils.latest_yolov2_snapshot(d, "paper")
    assert str(e.value) == ("--ckpt-dir %s holds snapshots of the darknet topology (train_iter_100.weights); this run trains "
                            "the paper topology, whose snapshots are .npz files" % d)
    p = str(tmp_path / "npz")
    os.makedirs(p)
    open(os.path.join(p, "train_iter_5.npz"), "wb").close()
    with pytest.raises(ValueError) as e:
        net_utils.latest_yolov2_snapshot(p, "tiny")
    assert str(e.value) == ("--ckpt-dir %s holds snapshots of the paper topology (train_iter_5.npz); this run trains the "
                            "tiny topology, whose snapshots are .weights files" % p)
    for f in (net_utils.save_yolov2_variables, net_utils.restore_yolov2_variables):
        with pytest.raises(ValueError) as e:
            f(Model("tiny"), "x.npz")
        assert "\"tiny\" topology are out of scope" in str(e.value)


def test_train_flags(tmp_path, capsys):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as T
    common = ["--devkit", "kit"]
    args = T.parse_args(common + ["--topology", "tiny"])
    assert args.topology == "tiny" and args.topology_stated == "tiny"
    assert T.TRAINERS["tiny"] is yolov2.YOLOv2DarknetTrainer
    args = T.parse_args(common + ["--darknet-weights", "f.weights"])
    assert args.topology == "darknet" and args.topology_stated is None          # until the file is read
    for bad in (["--topology", "tiny", "--imagenet-ckpt-dir", "d"], ["--topology", "paper", "--darknet-weights", "f"],
                ["--topology", "small"], ["--topology", "tiny", "--darknet-weights", "f", "--darknet-backbone", "g"]):
        with pytest.raises(SystemExit):
            T.parse_args(common + bad)
    capsys.readouterr()
    # --darknet-weights chooses the graph by the file; a stated topology that contradicts it is an argument error
    paths = {}
    for t in yolov2.DARKNET_FILE_TOPOLOGIES:
        paths[t] = str(tmp_path / (t + ".weights"))
        DW.write(paths[t], _random_layers(net_utils._file_layers(t, yolov2._TOPOLOGY[t].specs(20, 5, 8)), 5), 1)
    for t, other in (("tiny", "darknet"), ("darknet", "tiny")):
        assert T.file_topology(T.parse_args(common + ["--width-div", "8", "--darknet-weights", paths[t]]), 20) == t
        assert T.file_topology(T.parse_args(common + ["--width-div", "8", "--darknet-weights", paths[t], "--topology", t]),
                               20) == t
        with pytest.raises(SystemExit):
            T.file_topology(T.parse_args(common + ["--width-div", "8", "--darknet-weights", paths[t], "--topology", other]),
                            20)
        assert "holds the %s graph" % t in capsys.readouterr().err
    with pytest.raises(ValueError):
        T.file_topology(T.parse_args(common + ["--darknet-weights", paths["tiny"]]), 20)     # width_div 1: neither count


def test_eval_and_detect_flags(capsys):
    from tensorflow_yolo2_amd.pascal import pascal_detect_yolov2 as D, pascal_eval_yolov2 as EV
    for mod, base in ((EV, ["--devkit", "kit"]), (D, ["--images", "a.jpg"])):
        args = mod.parse_args(base + ["--darknet-weights", "tiny-yolo-voc.weights", "--protocol", "darknet"])
        assert args.darknet_weights == "tiny-yolo-voc.weights" and not hasattr(args, "topology")
        for bad in (["--darknet-weights", "f", "--weights", "x.npz"], ["--darknet-weights", "f", "--ckpt-dir", "d"],
                    ["--protocol", "darknet"]):
            with pytest.raises(SystemExit):
                mod.parse_args(base + bad)
        capsys.readouterr()
        with pytest.raises(SystemExit):
            mod.parse_args(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert "tiny-yolo-voc.cfg" in text and "float count" in text
