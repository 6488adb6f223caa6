"""Inputs shared by tests/test_wide_head_host.py and tests/test_gpu_wide_head.py: the 700-node tree that goes with
tests/golden/cfg/chain-wide.cfg, a copy of that cfg next to it, a random `.weights` file for its graph, the text of
YOLO9000's cfg as remembered, and the GEMM operands of the kernel parity.  Everything comes from fixed seeds on the CPU."""
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN_WIDE_CFG = os.path.join(ROOT, "tests", "golden", "cfg", "chain-wide.cfg")
CHAIN_TREE_CFG = os.path.join(ROOT, "tests", "golden", "cfg", "chain-tree.cfg")
WIDE_NODES = 700


def wide700_text():
    """700 nodes: 5 roots; 70 children of root 0 (a group wider than a wave); 10 of root 1; 20 of node 5 (depth 2); 15 of
    node 85 (depth 3); 8 of node 105 (depth 4); then 13 children each of nodes 6 .. 49 (depth 2): 50 groups in all"""
    lines = ["root%d -1" % i for i in range(5)]
    lines += ["a%d 0" % i for i in range(70)]               # nodes 5 .. 74
    lines += ["b%d 1" % i for i in range(10)]               # 75 .. 84
    lines += ["c%d 5" % i for i in range(20)]               # 85 .. 104
    lines += ["d%d 85" % i for i in range(15)]              # 105 .. 119
    lines += ["e%d 105" % i for i in range(8)]              # 120 .. 127
    for p in range(6, 50):
        lines += ["f%d_%d %d" % (p, i, p) for i in range(13)]
    assert len(lines) == WIDE_NODES
    return "\n".join(lines) + "\n"


def write_wide_model_files(tmp_path, with_map=True):
    """chain-wide.cfg (or, if not with_map, chain-wide-nomap.cfg: the same without its map= line) and wide700.tree in
    tmp_path -> the cfg's path"""
    tmp_path = str(tmp_path)
    cfg = os.path.join(tmp_path, "chain-wide.cfg" if with_map else "chain-wide-nomap.cfg")
    with open(CHAIN_WIDE_CFG) as f:
        text = f.read()
    if not with_map:
        assert text.count("map=x.map\n") == 1
        text = text.replace("map=x.map\n", "")
    with open(cfg, "w") as f:
        f.write(text)
    with open(os.path.join(tmp_path, "wide700.tree"), "w") as f:
        f.write(wide700_text())
    return cfg


def random_weights_file(path, file_layers, seed):
    """a Darknet `.weights` file for file_layers [(k, c, n, batch_norm)]: filters of standard deviation sqrt(2 / fan-in),
    batch-norm scales near 1 on rolling statistics (0, about 1), so activations stay of order 1 through the chain and the
    last layer's logits spread over a few units"""
    from tensorflow_yolo2_amd.utils import darknet_weights as dkw
    rng = np.random.default_rng(seed)
    layers = []
    for (k, c, n, bn) in file_layers:
        w = (rng.standard_normal((n, c, k, k)) * np.sqrt(2.0 / (c * k * k))).astype(np.float32)
        if bn:
            layers.append({"biases": (rng.standard_normal(n) * 0.1).astype(np.float32),
                           "scales": rng.uniform(0.8, 1.2, n).astype(np.float32),
                           "rolling_mean": (rng.standard_normal(n) * 0.1).astype(np.float32),
                           "rolling_variance": rng.uniform(0.5, 1.5, n).astype(np.float32), "weights": w})
        else:
            layers.append({"biases": (rng.standard_normal(n) * 0.5).astype(np.float32), "weights": w * np.float32(1.5)})
    dkw.write(path, layers, seen=1234)
    return path


# YOLO9000's layers as (filter size, filters, pool behind it): Darknet-19 without its classifier, then the 28,269-filter
# linear layer -- 19 convolutions
YOLO9000_CONVS = ((3, 32, 1), (3, 64, 1), (3, 128, 0), (1, 64, 0), (3, 128, 1), (3, 256, 0), (1, 128, 0), (3, 256, 1),
                  (3, 512, 0), (1, 256, 0), (3, 512, 0), (1, 256, 0), (3, 512, 1),
                  (3, 1024, 0), (1, 512, 0), (3, 1024, 0), (1, 512, 0), (3, 1024, 0))
YOLO9000_CLASSES, YOLO9000_NUM, YOLO9000_FILTERS = 9418, 3, 28269


def yolo9000_cfg_text():
    """yolo9000.cfg written down from memory of the published file (no copy was at hand): its [net] and [region] keys, its
    19 convolutions at full width"""
    out = ["[net]", "# Testing", "batch=1", "subdivisions=1", "# Training", "# batch=64", "# subdivisions=8", "height=544",
           "width=544", "channels=3", "momentum=0.9", "decay=0.0005", "", "learning_rate=0.001", "burn_in=1000",
           "max_batches = 500200", "policy=steps", "steps=400000,450000", "scales=.1,.1", "", "hue=.1", "saturation=.75",
           "exposure=.75", ""]
    for (k, n, pool) in YOLO9000_CONVS:
        out += ["[convolutional]", "batch_normalize=1", "filters=%d" % n, "size=%d" % k, "stride=1", "pad=1",
                "activation=leaky", ""]
        if pool:
            out += ["[maxpool]", "size=2", "stride=2", ""]
    out += ["[convolutional]", "filters=%d" % YOLO9000_FILTERS, "size=1", "stride=1", "pad=1", "activation=linear", ""]
    out += ["[region]", "anchors = 0.77871, 1.14074, 3.00525, 4.31277, 9.22725, 9.61974", "bias_match=1",
            "classes=%d" % YOLO9000_CLASSES, "coords=4", "num=%d" % YOLO9000_NUM, "softmax=1", "jitter=.2", "rescore=1", "",
            "object_scale=5", "noobject_scale=1", "class_scale=1", "coord_scale=1", "", "thresh = .6", "absolute=1",
            "random=1", "", "tree=data/9k.tree", "map = data/coco9k.map", ""]
    return "\n".join(out)


# (M, K, Cout) of the kernel parity: one ragged tile each way and one (half) K step; across 2048; the real M and K with a
# ragged odd Cout and several K steps; the smallest; the real width.  Then the regimes around them: exactly full tiles (no
# mask live); one row and one column into the second tiles; three row tiles and a half K step behind a full one; K at
# Y2_WIDE_HEAD_MAX_K; four row tiles x three panels through xcd_block; 72 rows in the second wave row, so that wave skips
# one of its four MFMA row tiles (three live)
GEMM_SHAPES = ((25, 32, 225), (147, 128, 2115), (289, 1024, 4099), (1, 64, 1), (300, 256, 28269),
               (256, 64, 256), (257, 64, 257), (513, 96, 300), (40, 4096, 260), (770, 160, 600), (200, 64, 33))
GUARD = 1024


def gemm_operands(M, K, Cout):
    """x [M][K], W [K][Cout], b [Cout] float32 with mixed signs and a spread of row magnitudes.  The parity gate bounds
    the accumulation error by sum_k |x_k w_k| and has no term for the one rounding of the bias add (2^-24 |out|), so the
    bias is kept of the order of that sum (standard deviation 0.1) instead of dominating it"""
    rng = np.random.default_rng(1000003 * M + 1009 * K + Cout)
    x = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-2, 2, (M, 1)))).astype(np.float32)
    W = (rng.standard_normal((K, Cout)) * 0.05).astype(np.float32)
    b = (rng.standard_normal(Cout) * 0.1).astype(np.float32)
    return x, W, b


def packed_image(lib, Wd, K, Cout):
    """y2_wide_head_pack of the device tensor Wd [K][Cout] into a buffer of exactly y2_wide_head_packed_bytes"""
    import ctypes
    import torch
    nbytes = lib.y2_wide_head_packed_bytes(K, Cout)
    assert nbytes == (Cout + 255) // 256 * 256 * ((K + 63) // 64 * 64) * 2
    packed = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.y2_wide_head_pack(ctypes.c_void_p(Wd.data_ptr()), K, Cout, ctypes.c_void_p(packed.data_ptr()), nbytes,
                                 None) == 0, lib.y2_last_error()
    return packed


def check_forward_on_the_device(x, W, b):
    """y2_wide_head_forward on one operand set against gemm_reference, the kernel parity of tests/test_gpu_wide_head.py:
    per element |got - ref| <= 2 K 2^-24 sum_k |x_k w_k| + 1e-30; the guard words behind out intact, a NaN prefill fully
    overwritten, two runs the same bits.  Needs the GPU; prints the figures before it asserts -> (got, ref, bound)"""
    import ctypes
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    (M, K), Cout = x.shape, W.shape[1]
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ref, mag = gemm_reference(x, W, b)
    xd, Wd, bd = dev(x), dev(W), dev(b)
    packed = packed_image(lib, Wd, K, Cout)
    runs = []
    for _ in range(2):
        buf = torch.full((M * Cout + GUARD,), float("nan"), device="cuda")
        guard = dev(np.random.default_rng(M).integers(-2 ** 31, 2 ** 31, GUARD).astype(np.int32))
        buf[M * Cout:].view(torch.int32).copy_(guard)
        assert lib.y2_wide_head_forward(p(xd), p(packed), p(bd), M, K, Cout, p(buf), None) == 0, lib.y2_last_error()
        torch.cuda.synchronize()
        assert torch.equal(buf[M * Cout:].view(torch.int32), guard)      # nothing behind out + M * Cout was written
        runs.append(buf[:M * Cout].cpu().numpy().reshape(M, Cout))
    got = runs[0]
    assert np.isfinite(got).all()                                        # every element was written
    assert np.array_equal(got.view(np.uint32), runs[1].view(np.uint32))  # two runs: the same bits
    bound = 2.0 * K * 2.0 ** -24 * mag + 1e-30
    ratio = np.abs(got.astype(np.float64) - ref) / bound
    print("wide head (%d, %d, %d): largest |got - ref| / bound = %.4f, largest |got - ref| = %.3e" %
          (M, K, Cout, ratio.max(), np.abs(got - ref).max()))
    assert ratio.max() <= 1.0, ratio.max()
    return got, ref, bound


def gemm_reference(x, W, b):
    """-> (float64 reference on the f16-rounded operands with the float32 bias, the bound's sum_k |x_k w_k|)"""
    xh, Wh = x.astype(np.float16).astype(np.float64), W.astype(np.float16).astype(np.float64)
    return xh @ Wh + b.astype(np.float64), np.abs(xh) @ np.abs(Wh)
