"""Training the wide head on the host (no GPU): the split plan of csrc/wide_head_train.hip over a table of shapes, its
workspace sizes, the loader that admits either kind of cfg, from_cfg's keyword on the record level and the data-parallel
refusal."""
import ctypes

import pytest

import _wide_head_cases as K

SHAPES = ((1, 64, 1), (25, 32, 225), (256, 64, 256), (257, 64, 257), (513, 96, 300), (40, 1024, 515), (147, 128, 2115),
          (300, 256, 28269), (289, 1024, 28269), (9248, 1024, 28269), (50, 128, 28269), (100000, 4096, 65536 * 16))
MAX_SPLIT = 64


def up(a, b):
    return (a + b - 1) // b


def plan(lib, M, Kdim, Cout, cus):
    a, b = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.y2_wide_head_train_plan(M, Kdim, Cout, cus, ctypes.byref(a), ctypes.byref(b)) == 0, lib.y2_last_error()
    return a.value, b.value


def test_plan_split_counts_over_a_table_of_shapes():
    """per product: at least one split, at most 64 and at most the reduction steps; every split holds a step (the count
    is ceil(steps / ceil(steps / n)) of itself); one split where the tiles alone fill the device; never more workgroups
    than one tile past the device unless the tiles alone exceed it; non-decreasing in the CU count"""
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    for (M, Kdim, Cout) in SHAPES:
        last = (1, 1)
        for cus in (1, 8, 64, 104, 256, 304, 1024):
            got = plan(lib, M, Kdim, Cout, cus)
            for split, tiles, steps in ((got[0], up(M, 128) * up(Kdim, 128), up(Cout, 64)),
                                        (got[1], up(Kdim, 128) * up(Cout, 128), up(M, 64))):
                assert 1 <= split <= min(MAX_SPLIT, steps), (M, Kdim, Cout, cus, split)
                assert split == up(steps, up(steps, split))
                if tiles >= cus:
                    assert split == 1
                else:
                    assert split <= up(cus, tiles)
            assert got[0] >= last[0] and got[1] >= last[1], (M, Kdim, Cout, cus)
            last = got
    # the shapes of the issue on an MI355X's 256 CUs: 3 x 8 tiles share 442 steps 11 ways; 8 x 221 tiles need no split
    assert plan(lib, 289, 1024, 28269, 256) == (11, 1)
    assert plan(lib, 9248, 1024, 28269, 256) == (1, 1)
    assert plan(lib, 300, 256, 28269, 256)[0] > 1 and 442 % up(442, plan(lib, 300, 256, 28269, 256)[0]) != 0   # ragged last split


def test_workspace_bytes_follow_the_split():
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    for (M, Kdim, Cout) in SHAPES[:9]:
        steps_x, steps_w = up(Cout, 64), up(M, 64)
        for split in (1, 2, 3, 5, 64, 1000):
            nx = min(split, MAX_SPLIT, steps_x)
            nx = up(steps_x, up(steps_x, nx))
            nw = min(split, MAX_SPLIT, steps_w)
            nw = up(steps_w, up(steps_w, nw))
            assert lib.y2_wide_head_backward_input_workspace_bytes(M, Kdim, Cout, split) == (nx * M * Kdim * 4 if nx > 1 else 0)
            assert lib.y2_wide_head_backward_filter_workspace_bytes(M, Kdim, Cout, split) == (nw * Kdim * Cout * 4 if nw > 1 else 0)
        assert lib.y2_wide_head_backward_input_workspace_bytes(M, Kdim, Cout, -1) == 0
    assert lib.y2_wide_head_packed2_bytes(1024, 28269) == 1024 * 28288 * 2
    assert lib.y2_wide_head_packed2_bytes(96, 300) == 128 * 320 * 2


def test_load_graph_admits_a_wide_cfg_and_keeps_every_other_refusal(tmp_path):
    from tensorflow_yolo2_amd.utils import darknet_cfg as C
    record, graph, wide = C.load_graph(K.write_wide_model_files(tmp_path))
    assert wide is True and graph.wide and record.map == "x.map" and graph.file_layers[-1] == (1, 128, 2115, False)
    record, graph, wide = C.load_graph(K.write_wide_model_files(tmp_path, with_map=False))
    assert wide is True and graph.wide and record.map is None
    record, graph, wide = C.load_graph(K.CHAIN_TREE_CFG)
    assert wide is False and not graph.wide and record == C.load(K.CHAIN_TREE_CFG)
    # a narrow model that names a map keeps the default keyword's refusal
    with open(K.CHAIN_TREE_CFG) as f:
        text = f.read()
    assert text.count("[region]\n") == 1
    bad = tmp_path / "narrow-map.cfg"
    bad.write_text(text.replace("[region]\n", "[region]\nmap=x.map\n"))
    with pytest.raises(ValueError, match="map=x.map"):
        C.load_graph(str(bad))


def test_cfg_topology_keyword_on_the_record_level(tmp_path):
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    cfg = K.write_wide_model_files(tmp_path)
    topo, record = yolov2._cfg_topology(cfg, "f16", True, training=True)
    assert topo.wide == (128, 2115) and topo.name == "tiny" and record.map == "x.map"
    assert topo.slopes[-1] == [0.1, 0.1] and "core_layers" not in topo.train_options[-1]   # an ordinary head stack
    assert yolov2._cfg_topology(cfg, "fp8", True)[0].wide == (128, 2115)                   # the detector's mode stays
    for dtype in ("f32", "bf16", "f16x2", "f16x2f", "fp8"):
        with pytest.raises(ValueError) as e:
            yolov2._cfg_topology(cfg, dtype, True, training=True)
        assert "dtype %r" % dtype in str(e.value) and "'f16' only" in str(e.value)
    with pytest.raises(ValueError, match="map"):
        yolov2._cfg_topology(cfg, "f16", False, training=True)           # the default keyword: today's refusal
    import inspect
    assert inspect.signature(yolov2.YOLOv2DarknetTrainer.from_cfg).parameters["wide_head"].default is False


def test_the_train_script_loads_a_wide_cfg_with_the_keyword_by_itself(tmp_path, capsys):
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as T
    cfg = K.write_wide_model_files(tmp_path)
    args = T.parse_args(["--cfg", cfg], need_devkit=False)
    assert args.wide_head is True and args.topology == "tiny" and args.dtype == "f16" and args.solver == "darknet"
    assert args.cfg_record.map == "x.map" and args.cfg_graph.wide and args.tree_record.n == 700
    assert T.parse_args(["--cfg", K.CHAIN_TREE_CFG], need_devkit=False).wide_head is False
    with pytest.raises(SystemExit):
        T.parse_args(["--cfg", cfg, "--dtype", "f32"], need_devkit=False)
    assert "wide head (2115 filters), which trains under --dtype f16 only" in capsys.readouterr().err


def test_a_wide_head_refuses_data_parallel_training(monkeypatch):
    from tensorflow_yolo2_amd import trainer
    from tensorflow_yolo2_amd.yolo2_nets import yolov2

    class Dist:
        def __init__(self, world):
            self.world = world

        def get_world_size(self):
            return self.world

    class Topo:
        wide = (1024, 28269)

    tr = object.__new__(yolov2.YOLOv2DarknetTrainer)
    tr._topo = Topo()
    monkeypatch.setattr(trainer, "_dist", lambda: Dist(2))
    with pytest.raises(ValueError, match="world size 2"):
        tr._refuse_wide_replicas()
    monkeypatch.setattr(trainer, "_dist", lambda: Dist(1))              # a forced single-rank group
    tr._refuse_wide_replicas()
    monkeypatch.setattr(trainer, "_dist", lambda: None)
    tr._refuse_wide_replicas()
