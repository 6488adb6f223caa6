"""csrc/word_tree.hip and csrc/wide_head.hip at the width of the one model they exist for: YOLO9000's 9,418 tree nodes, rows
of 9,423 floats and 28,269 filters (inputs: tests/_yolo9000_cases.py; their conditions are asserted on the host by
tests/test_yolo9000_cases_host.py and again here before any device call).

What only this width runs: phase B of the tree loss with a row longer than the workgroup's stride (D > 256: dr = 0), lane
strides of up to 17 turns over one group, walks of 15 levels, groups of 63 / 64 / 65 / 129 / 1 members, and the whole
detector behind a (128, 28269) wide head under both storage modes.  The GEMM regimes around the tile sizes are further
cases of tests/test_gpu_wide_head.py (tests/_wide_head_cases.py GEMM_SHAPES); here are the operands in f16's subnormal range.
The checks and the gates are those of tests/test_gpu_word_tree.py and tests/test_gpu_wide_head.py, unchanged: loss rtol
2e-5, largest gradient error / largest gradient < 2e-5, statistics and prob rtol 2e-5, GEMM |got - ref| <= 2 K 2^-24
sum |x w| + 1e-30."""
import numpy as np
import pytest

import _wide_head_cases as WH
import _word_tree_cases as WT
import _yolo9000_cases as Y
from tensorflow_yolo2_amd.utils import detect_batch as DB, word_tree as W

gpu = pytest.mark.gpu
MARGIN = WT.MARGIN


def dev(a):
    import torch
    return torch.as_tensor(np.array(a)).cuda()


def bits(t):
    return t.cpu().numpy().view(np.uint32)


@gpu
@pytest.mark.parametrize("key", sorted(Y.SHAPES))
def test_tree_loss_matches_the_float64_specification_across_two_workgroups(key):
    """300 slots: two workgroups per image, the second with 44 live slots; D = 9,423 (big) and 75 (wide: 256 % 75 != 0).
    The zero check over 2 x 300 x D floats and the NaN-filled buffer are what see phase B's stepping"""
    WT.check_tree_loss_on_the_device(Y.parity_input(key))


@gpu
def test_tree_stats_match_the_float64_specification_at_9418_nodes():
    WT.check_tree_stats_on_the_device(Y.parity_input("n2_S10_B3_big"))


@gpu
@pytest.mark.parametrize("thresh", Y.HEAD_THRESHOLDS)
def test_word_tree_head_matches_the_specification_at_9418_nodes(thresh):
    import torch
    from tensorflow_yolo2_amd import engine as E
    net, tree = Y.head_rows()
    assert net.shape[0] % 4                                              # not a multiple of a workgroup's rows
    ref_out, ref_top, ref_prob, m = W.word_tree_head(net, tree, thresh, return_margins=True)
    assert m["thresh"] >= MARGIN and m["group_gap"] >= MARGIN, m
    if thresh == Y.DEPTH_THRESH:
        assert set(tree.depth[ref_top].tolist()) == set(range(15))
    tt = E.WordTreeTables(tree)
    src = dev(net)
    out = torch.full(net.shape, 7.0, device="cuda")
    got, top, prob = E.word_tree_head(src, tt, thresh, out=out, want_top=True)
    assert got is out and np.array_equal(bits(src), net.view(np.uint32))  # the input is not written
    o = out.cpu().numpy()
    assert np.array_equal(top.cpu().numpy(), ref_top)
    assert np.array_equal(o.view(np.uint32), ref_out.view(np.uint32))    # boxes copied, +0.0 at top, -inf elsewhere
    err = np.abs(prob.cpu().numpy() - ref_prob) / ref_prob
    print("word_tree_head 9418 nodes thresh %.1f: largest relative error of prob %.3e" % (thresh, err.max()))
    np.testing.assert_allclose(prob.cpu().numpy(), ref_prob, rtol=2e-5)
    # in place, and without the optional outputs: the same bits
    same = E.word_tree_head(src, tt, thresh, out=src)
    assert same is src and np.array_equal(bits(src), bits(out))


@gpu
def test_forward_keeps_f16_subnormal_operands():
    """the kernel's contract is f16(x[m][k]) * f16(W[k][c]): a flush of subnormals in the convert, the pack or the matrix
    pipe would return 0 for most of these products"""
    x, Wt, b = Y.gemm_operands_subnormal(*Y.SUBNORMAL_SHAPE)
    assert Y.subnormal_share(x) >= 0.5 and Y.subnormal_share(Wt) >= 0.5
    got, ref, bound = WH.check_forward_on_the_device(x, Wt, b)
    clear = np.abs(ref) > 100.0 * bound
    print("subnormal operands: %.3f of the elements have |ref| > 100 bound; zeros among them: %d" %
          (clear.mean(), (got[clear] == 0).sum()))
    assert clear.mean() > 0.9 and (got[clear] != 0).all()


@gpu
@pytest.mark.parametrize("dtype", ["f16", "fp8"])
def test_detector_with_28269_filters_end_to_end(tmp_path, monkeypatch, dtype):
    """chain-wide.cfg with YOLO9000's head (filters=28269, classes=9418, the big tree) at 160 x 160 (S = 5), batch 2: the
    chain of tests/test_gpu_wide_head.py's end-to-end test, every check relative to the device's own head-stack output;
    and the raw head against float64 on that output's f16 rounding and the loaded filters.  That gate has no term for the
    rounding of the bias add, 2^-24 |out|; it is covered here because |bias| (standard deviation 0.5) is far below
    K sum |x w| (sum |x w| is of order 10).
    fp8: the shipped plan admits no layer shape of this chain to the MXFP8 kernel (the mode is f16
    there), so the case sets the plan's switch Y2_MX8_ALL=1 as tests/test_gpu_fp8_inference.py does, and asserts that the
    stack in front of the wide head then differs from the f16 model's"""
    import torch
    from test_gpu_detect_anchor import SHAPES, _table
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    n, S, thresh, iou, max_out, D = 2, 5, 0.05, 0.45, 20, 5 + Y.NODES
    cfg = Y.write_yolo9000_width_files(tmp_path)
    if dtype == "fp8":
        monkeypatch.setenv("Y2_MX8_ALL", "1")                            # read when the stacks are created
    det = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype=dtype, seed=3, wide_head=True,
                                         tree_thresh=Y.DETECTOR_TREE_THRESH)
    assert det.wide is not None and (det.wide.K, det.wide.Cout) == (128, 28269)
    assert det.tree is not None and det.tree.n == 9418 == det.num_class and det.B == 3 and det.tree.max_depth == 14
    # load -> save: the bytes read
    src = WH.random_weights_file(str(tmp_path / "wide.weights"), det.cfg.file_layers, seed=Y.DETECTOR_WEIGHTS_SEED)
    assert net_utils.load_darknet_weights(det, src) == 1234
    back = str(tmp_path / "back.weights")
    net_utils.save_darknet_weights(det, back, 1234)
    with open(src, "rb") as f, open(back, "rb") as g:
        data = f.read()
        assert data == g.read() and len(data) == 16 + 4 * det.cfg.floats
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8))
    table = torch.from_numpy(_table()).cuda()
    raw = torch.full((n, S, S, 3, D), float("nan"), device="cuda")
    d, s, c = det.detect_batch(x, table, None, thresh, iou, max_out, grid_out=raw)
    torch.cuda.synchronize()
    # the raw head is the wide operator on the head stack's own output, bit for bit
    stack_out = det.head._out
    assert tuple(stack_out.shape) == (n, S, S, 128) and stack_out.dtype == torch.float32
    again = det.wide.forward(stack_out, out=torch.empty(n * S * S * 28269, device="cuda"))
    assert np.array_equal(again.cpu().numpy().view(np.uint32), raw.cpu().numpy().view(np.uint32).ravel())
    head = raw.cpu().numpy().reshape(-1, D)
    assert np.isfinite(head).all() and head[:, 5:].std() > 0.3
    # ... and float64 on the f16-rounded stack output and the loaded filters, within the GEMM bound
    filters = det.wide.export()
    ref, mag = WH.gemm_reference(stack_out.cpu().numpy().reshape(n * S * S, 128), filters["W"].reshape(128, 28269), filters["b"])
    ratio = np.abs(raw.cpu().numpy().reshape(n * S * S, 28269).astype(np.float64) - ref) / (2.0 * 128 * 2.0 ** -24 * mag + 1e-30)
    print("detector %s (50, 128, 28269): largest |got - ref| / bound = %.4f, logits' std %.3f" % (dtype, ratio.max(),
                                                                                                  head[:, 5:].std()))
    assert ratio.max() <= 1.0, ratio.max()
    # the host specification from the device's raw head: the tree walk, then the rows
    spec_head, top, _prob, m = W.word_tree_head(head, det.tree.tree, det.tree_thresh, return_margins=True)
    assert m["thresh"] >= MARGIN and m["group_gap"] >= MARGIN, m
    print("detector %s: %d distinct nodes among %d rows, deepest %d" % (dtype, len(set(top.tolist())), len(top),
                                                                        det.tree.tree.depth[top].max()))
    assert len(set(top.tolist())) > 10 and det.tree.tree.depth[top].max() >= 1
    boxes, scores = E.decode_anchors(dev(spec_head.astype(np.float32).reshape(n, S, S, 3, D)), det.anchors)
    best, cls = E.class_argmax(scores)
    boxes, best, cls = (t.cpu().numpy() for t in (boxes, best, cls))
    assert np.array_equal(cls.ravel(), top)
    d, s, c = d.cpu().numpy(), s.cpu().numpy(), c.cpu().numpy()
    for k in range(n):
        want_det, want_score = DB.anchor_detect(boxes[k], best[k], cls[k], SHAPES[k][1], SHAPES[k][0], thresh, iou, max_out)
        cnt = len(want_det)
        assert c[k] == cnt and np.array_equal(d[k, :cnt], want_det), k
        assert np.array_equal(s[k, :cnt].view(np.uint32), want_score.view(np.uint32)), k
        assert (d[k, cnt:] == -1).all() and (s[k, cnt:] == 0).all()
    assert c.sum() > 0
    # detect() reads the same head
    _b, _best, cls2, _keep, _count = det.detect(x)
    assert np.array_equal(cls2.cpu().numpy().ravel(), top)
    if dtype == "fp8":
        twin = yolov2.YOLOv2Detector.from_cfg(cfg, n, image_size=160, dtype="f16", seed=3, wide_head=True,
                                              tree_thresh=Y.DETECTOR_TREE_THRESH)
        net_utils.load_darknet_weights(twin, src)
        twin.detect_batch(x, table, None, thresh, iou, max_out)
        diff = (twin.head._out - stack_out).abs().max().item() / stack_out.abs().max().item()
        print("detector fp8: the head stack's output differs from the f16 model's by %.3e of its maximum" % diff)
        assert diff > 0.0
