"""What YOLO9000's last layer and what follows it cost: K = 1024, Cout = 28,269 (3 anchors x (5 + 9,418 nodes)), one 544 x
544 image (M = 289 cells) and a batch of 32 (M = 9,248):

  (a) wide head   y2_wide_head_forward: fp32 x converted in the kernel, packed f16 filters, fp32 out + bias
  (b) yardstick   torch.addmm(bias, x16, W16) on f16 copies of the same operands, then .float(): the vendor GEMM of this
                  box, the GEMM ceiling scripts/gemm_ceiling.py already uses; its conversion of x is NOT in the timing
  (c) tree head   engine.word_tree_head on (a)'s result into a second buffer, a generated 9,418-node tree
  (d) detect      engine.detect_anchor_batch on that head

The expectation written down before measuring: (a) is no slower than (b) by more than 10 % -- twice the README's +-4 %
box-to-box spread plus the bias and the conversion that (b) does not do the same way.  An expectation, not a gate.

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported (a leg whose single call takes longer than 25 ms runs in blocks of 2).  Bytes of (a): the packed
filters once, x once, out once.  FLOP: 2 M K Cout.  Also here: the largest |got - ref| / bound of the kernel parity at the
shapes of tests/test_gpu_wide_head.py.

    python scripts/bench_wide_head.py --out profiles/wide_head.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STREAM_TBS = 5.0                    # what the streaming kernels of this library reach
F16_PEAK_PF = 2.5                   # dense f16 MFMA peak
PARITY_SHAPES = ((25, 32, 225), (147, 128, 2115), (289, 1024, 4099), (1, 64, 1), (300, 256, 28269))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--cout", type=int, default=28269)
    ap.add_argument("--cells", type=int, default=289)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--anchors", type=int, default=3)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from bench_word_tree import generated_tree
    from tensorflow_yolo2_amd import engine as E
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def block_us(fn, inner):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) * 1e3 / inner

    def medians(legs):
        inner = {}
        for name, fn in legs:
            fn()
            torch.cuda.synchronize()
            inner[name] = args.inner if block_us(fn, 1) < 25e3 else 2
        us = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                us[name].append(block_us(fn, inner[name]))
        return {k: statistics.median(v) for k, v in us.items()}, inner

    Kd, Cout, B = args.k, args.cout, args.anchors
    assert Cout % B == 0
    Cn = Cout // B - 5
    rng = np.random.default_rng(0)
    Wt = (rng.standard_normal((Kd, Cout), np.float32) * np.float32(0.05))
    bias = rng.standard_normal(Cout, np.float32) * np.float32(0.5)
    wide = E.WideHead(Kd, Cout)
    wide.load(Wt, bias)
    W16 = torch.from_numpy(Wt).cuda().half()
    b16 = torch.from_numpy(bias).cuda().half()
    tree = E.WordTreeTables(generated_tree(Cn, args.depth))
    anchors = torch.as_tensor(np.asarray(((0.77871, 1.14074), (3.00525, 4.31277), (9.22725, 9.61974))[:B], np.float32)).cuda()
    say("Wide head, K = %d, Cout = %d (%d anchors x (5 + %d nodes in %d groups, depth %d)); HIP events, median of %d "
        "alternating blocks of %d calls, microseconds per call; bytes against %.1f TB/s, FLOP against %.1f PF"
        % (Kd, Cout, B, Cn, tree.groups, tree.max_depth, args.reps, args.inner, STREAM_TBS, F16_PEAK_PF))
    say("    M  GFLOP  MB filters + x + out  us at %.0f TB/s  us at %.1f PF  (a) wide head  TB/s   PF    (b) addmm f16 + float  "
        "(a)/(b)  (c) tree head  (d) detect" % (STREAM_TBS, F16_PEAK_PF))
    for batch in [int(v) for v in args.batches.split(",")]:
        M = batch * args.cells
        S = int(round(args.cells ** 0.5))
        assert S * S == args.cells
        x = torch.from_numpy(rng.standard_normal((M, Kd), np.float32)).cuda()
        x16 = x.half()
        out = torch.empty((M, Cout), dtype=torch.float32, device="cuda")
        table = torch.from_numpy(np.array([(0, 375, 500, 1504, 0)] * batch, np.int64)).cuda()
        det = (torch.empty((batch, 100, 6), dtype=torch.int32, device="cuda"),
               torch.empty((batch, 100), dtype=torch.float32, device="cuda"),
               torch.empty((batch,), dtype=torch.int32, device="cuda"))
        grid = out.view(batch, S, S, B, 5 + Cn)
        head = torch.empty_like(grid)
        keep = {}

        def a():
            wide.forward(x, out=out)

        def b():
            keep["b"] = torch.addmm(b16, x16, W16).float()

        def c():
            E.word_tree_head(grid, tree, 0.5, out=head)

        def d():
            E.detect_anchor_batch(head, anchors, table, None, 0.005, 0.45, 100, out=det)

        med, inner = medians([("a", a), ("b", b)])
        a()
        c()                              # (c) reads (a)'s raw head, (d) the rewritten one
        more, inner2 = medians([("c", c), ("d", d)])
        med.update(more)
        inner.update(inner2)
        gflop = 2.0 * M * Kd * Cout / 1e9
        mb = (wide.packed.numel() + M * Kd * 4 + M * Cout * 4) / 1e6
        say("%5d  %5.1f  %20.1f  %13.1f  %12.1f  %13.1f  %4.2f  %4.2f  %23.1f  %7.2f  %13.1f  %10.1f%s"
            % (M, gflop, mb, mb / STREAM_TBS, gflop / F16_PEAK_PF, med["a"], mb / med["a"], gflop / med["a"],
               med["b"], med["a"] / med["b"], med["c"], med["d"],
               "".join("  [(%s): blocks of %d]" % (k, v) for k, v in sorted(inner.items()) if v != args.inner)))
        del keep, x16, out, grid, head
    say()
    say("Kernel parity, y2_wide_head_forward against numpy float64 on the f16-rounded operands: largest |got - ref| / "
        "(2 K 2^-24 sum_k |x_k w_k| + 1e-30) per shape (the gate of tests/test_gpu_wide_head.py is 1)")
    say("    M     K   Cout  ratio")
    for (M, Kp, Cp) in PARITY_SHAPES:
        r = np.random.default_rng(1000003 * M + 1009 * Kp + Cp)
        x = (r.standard_normal((M, Kp)) * np.exp(r.uniform(-2, 2, (M, 1)))).astype(np.float32)
        Wp = (r.standard_normal((Kp, Cp)) * 0.05).astype(np.float32)
        bp = (r.standard_normal(Cp) * 0.1).astype(np.float32)
        op = E.WideHead(Kp, Cp)
        op.load(Wp, bp)
        got = op.forward(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
        xh, Wh = x.astype(np.float16).astype(np.float64), Wp.astype(np.float16).astype(np.float64)
        bound = 2.0 * Kp * 2.0 ** -24 * (np.abs(xh) @ np.abs(Wh)) + 1e-30
        say("%5d  %4d  %5d  %.4f" % (M, Kp, Cp, (np.abs(got - (xh @ Wh + bp.astype(np.float64))) / bound).max()))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
