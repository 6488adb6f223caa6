"""What training the graph of yolov2-voc.cfg costs (yolo2_nets/yolov2.py: YOLOv2DarknetTrainer; csrc/ext.hip:
y2_passthrough_concat_darknet_backward), one MI355X, the method of scripts/bench_darknet_yolov2.py:

  (b) / (f) / (s)   y2_passthrough_concat_darknet_backward / y2_passthrough_concat_darknet (the same bytes in the other
                    direction) / y2_passthrough_concat_backward (the space-to-depth gradient) at Cf = 64, Cc = 1024,
                    S = 13 and 19, batch --kernel-batch (32): ms and GB/s each, and the ratios
  (k) / (p)         one f16 train step, YOLOv2DarknetTrainer / YOLOv2Trainer, 416 x 416, batch --step-batch (64), box
                    labels, Darknet's SGD solver

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  Nothing is claimed beforehand: the ratios are the result.

    python scripts/bench_darknet_train.py --out profiles/darknet_train.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-batch", type=int, default=32)
    ap.add_argument("--step-batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils.solver import Solver
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def block_ms(fn, inner):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / inner

    def medians(legs, inner, warm=1):
        for _ in range(warm):                                    # warm-up: kernel loads, filter packs, optimizer state
            for _name, fn in legs:
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                ms[name].append(block_ms(fn, inner))
        return {k: statistics.median(v) for k, v in ms.items()}

    rng = np.random.default_rng(0)
    n = args.kernel_batch
    say("Training Darknet's YOLOv2 graph beside the paper's; HIP events, median of %d alternating blocks, milliseconds per "
        "call (blocks of %d launches, of %d steps)" % (args.reps, 20 * args.inner, args.inner))
    cf, cc = 64, 1024
    for S in (13, 19):
        fine = torch.from_numpy(rng.standard_normal((n, 2 * S, 2 * S, cf)).astype(np.float32)).cuda()
        coarse = torch.from_numpy(rng.standard_normal((n, S, S, cc)).astype(np.float32)).cuda()
        dout = torch.from_numpy(rng.standard_normal((n, S, S, 4 * cf + cc)).astype(np.float32)).cuda()
        out = torch.empty_like(dout)
        dfine, dcoarse = torch.empty_like(fine), torch.empty_like(coarse)
        lib = E._lib.load()

        def backward():
            E.passthrough_concat_darknet_backward(dout, cf, dfine_out=dfine, dcoarse_out=dcoarse)

        def forward():
            E.passthrough_concat_darknet(fine, coarse, out=out)

        def plain():
            E.check(lib.y2_passthrough_concat_backward(E._ptr(dout), E._ptr(dfine), E._ptr(dcoarse), n, S, S, cf, cc,
                                                       E._stream()))

        med = medians([("b", backward), ("f", forward), ("s", plain)], inner=20 * args.inner)
        moved = 2 * dout.numel() * 4                             # every value read once and written once, all three
        gbs = lambda k: moved / med[k] / 1e6
        say("batch %d  S %2d  Cf %d  Cc %d  %.1f MB moved  (b) darknet backward %.4f ms %.0f GB/s  (f) darknet forward %.4f "
            "ms %.0f GB/s  (s) space-to-depth backward %.4f ms %.0f GB/s  (b)/(f) %.3f  (b)/(s) %.3f" %
            (n, S, cf, cc, moved / 1e6, med["b"], gbs("b"), med["f"], gbs("f"), med["s"], gbs("s"), med["b"] / med["f"],
             med["b"] / med["s"]))
    if not args.no_step:
        n, size = args.step_batch, args.size
        images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
        truth = np.zeros((n, 30, 5), np.float32)
        for i in range(n):
            for j in range(2):
                w, h = rng.uniform(0.1, 0.5, 2) * size
                truth[i, j] = (rng.uniform(0.3, 0.7) * size, rng.uniform(0.3, 0.7) * size, w, h, rng.integers(0, 20))
        truth = torch.from_numpy(truth).cuda()
        ntruth = torch.full((n,), 2, dtype=torch.int32, device="cuda")
        kw = dict(dtype=args.dtype, width_div=args.width_div, solver=Solver())
        paper = yolov2.YOLOv2Trainer(n, size, **kw)
        dark = yolov2.YOLOv2DarknetTrainer(n, size, **kw)
        med = medians([("p", lambda: paper.step(images, truth=truth, ntruth=ntruth)),
                       ("k", lambda: dark.step(images, truth=truth, ntruth=ntruth))], inner=args.inner, warm=3)
        fp, fk = paper.flops_per_step(size), dark.flops_per_step(size)
        say("batch %d  size %d  %s train step, box labels, DarknetSGD  (p) paper %.3f ms  (k) darknet %.3f ms  (k)/(p) %.3f  "
            "(p)-(k) %.3f ms;  algorithmic FLOPs per step (p) %.3e  (k) %.3e  (k)/(p) %.3f" %
            (n, size, args.dtype, med["p"], med["k"], med["k"] / med["p"], med["p"] - med["k"], fp, fk, fk / fp))
        for name, tr in (("p", paper), ("k", dark)):
            fin = all(bool(torch.isfinite(net.params).all()) for net in tr.networks())
            say("  (%s) parameters finite after the run: %s; steps skipped by the overflow guard: %d" %
                (name, fin, tr.opts[0].scaler.state()[2] if tr.opts[0].scaler is not None else 0))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
