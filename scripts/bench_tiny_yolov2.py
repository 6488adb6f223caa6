"""What the "tiny" topology (tiny-yolo-voc.cfg; yolo2_nets/yolov2.py) and its stride-1 pool (csrc/ext.hip: y2_maxpool2x2s1,
y2_maxpool2x2s1_backward) cost, one MI355X, the method of scripts/bench_darknet_train.py:

  (f) / (b)         y2_maxpool2x2s1 / y2_maxpool2x2s1_backward on (batch, S, S, 512), S = 13 and 19, batch --kernel-batch
                    (32), beside (F) / (B) y2_maxpool2x2 / y2_maxpool2x2_backward on (batch, 26, 26, 512) in the same
                    process: ms and GB/s of the bytes each must move -- forward: the input read once, the output written
                    once; backward: x and dy read once, dx written once.  The working sets fit the last-level cache: these
                    are cache rates.
  (t) / (k)         the detector's forward pass, f16, batch --forward-batch (32), "tiny" / "darknet", 416 x 416
  (T) / (K)         one f16 train step, YOLOv2DarknetTrainer "tiny" / "darknet", batch --step-batch (64), box labels,
                    Darknet's SGD solver, 416 x 416
  padding           the time of stack layers 0 and 1 within the tiny forward and step, from the per-layer events
                    (Network.profile_enable(1): every launch bracketed, serialised): the two layers run 32 wide where the
                    file holds 16 filters and 16 input channels, so at most half of this is what native kernels could save

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  Nothing is claimed beforehand.

    python scripts/bench_tiny_yolov2.py --out profiles/tiny_yolov2.txt
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
    ap.add_argument("--forward-batch", type=int, default=32)
    ap.add_argument("--step-batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--no-model", action="store_true")
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
    lib = E._lib.load()
    n, c = args.kernel_batch, 512
    say("Darknet's stride-1 pool and the tiny topology; HIP events, median of %d alternating blocks, milliseconds per call "
        "(blocks of %d launches, of %d passes)" % (args.reps, 20 * args.inner, args.inner))
    rand = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).cuda()
    big = rand(n, 26, 26, c)
    big_y = torch.empty((n, 13, 13, c), dtype=torch.float32, device="cuda")
    big_dy, big_dx = rand(n, 13, 13, c), torch.empty_like(big)
    p, st = E._ptr, E._stream
    for S in (13, 19):
        x, dy = rand(n, S, S, c), rand(n, S, S, c)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        legs = [("f", lambda: E.check(lib.y2_maxpool2x2s1(p(x), p(y), n, S, S, c, st()))),
                ("b", lambda: E.check(lib.y2_maxpool2x2s1_backward(p(x), p(dy), p(dx), n, S, S, c, st()))),
                ("F", lambda: E.check(lib.y2_maxpool2x2(p(big), p(big_y), n, 26, 26, c, st()))),
                ("B", lambda: E.check(lib.y2_maxpool2x2_backward(p(big), p(big_dy), p(big_dx), n, 26, 26, c, st())))]
        med = medians(legs, inner=20 * args.inner)
        moved = {"f": 2 * x.numel() * 4, "b": 3 * x.numel() * 4, "F": (big.numel() + big_y.numel()) * 4,
                 "B": (2 * big.numel() + big_dy.numel()) * 4}
        gbs = {k: moved[k] / med[k] / 1e6 for k in med}
        say("batch %d  C %d  (f) stride-1 forward  S %2d  %.1f MB  %.4f ms %.0f GB/s   (F) 2x2/2 forward  26 -> 13  %.1f MB  "
            "%.4f ms %.0f GB/s   rate (f)/(F) %.3f" %
            (n, c, S, moved["f"] / 1e6, med["f"], gbs["f"], moved["F"] / 1e6, med["F"], gbs["F"], gbs["f"] / gbs["F"]))
        say("batch %d  C %d  (b) stride-1 backward S %2d  %.1f MB  %.4f ms %.0f GB/s   (B) 2x2/2 backward 26 <- 13  %.1f MB  "
            "%.4f ms %.0f GB/s   rate (b)/(B) %.3f" %
            (n, c, S, moved["b"] / 1e6, med["b"], gbs["b"], moved["B"] / 1e6, med["B"], gbs["B"], gbs["b"] / gbs["B"]))
    if args.no_model:
        return finish(args, lines)

    def flops_forward(specs, heights, batch, size):
        tot = 0.0
        for spec, units in zip(specs, heights):
            h = units * (size // 32)
            for (k, ci, co, pool) in spec:
                tot += 2.0 * batch * h * h * k * k * ci * co
                if pool:
                    h = (h + 1) // 2
        return tot

    def layer_ms(net, fn, passes):
        """per-layer milliseconds [layers][categories] of `passes` calls of fn, every launch of `net` bracketed"""
        net.profile_enable(1)
        for _ in range(passes):
            fn()
        torch.cuda.synchronize()
        a = net.profile_layers() / passes
        net.profile_collect()
        net.profile_enable(0)
        return a

    size = args.size
    # ---- forward
    n = args.forward_batch
    images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
    tiny = yolov2.YOLOv2Detector(n, size, anchors=yolov2.ANCHORS_TINY_VOC, dtype=args.dtype, width_div=args.width_div,
                                 topology="tiny")
    dark = yolov2.YOLOv2Detector(n, size, dtype=args.dtype, width_div=args.width_div, topology="darknet")
    med = medians([("t", lambda: tiny.forward(images)), ("k", lambda: dark.forward(images))], inner=args.inner, warm=3)
    ft = flops_forward(tiny._topo.specs(20, 5, args.width_div), tiny._topo.heights, n, size)
    fk = flops_forward(dark._topo.specs(20, 5, args.width_div), dark._topo.heights, n, size)
    # the file's widths: what Darknet computes for the two narrow layers (16 filters, 16 input channels)
    ft_file = ft - 2.0 * n * size * size * 9 * 3 * 16 - 2.0 * n * (size // 2) ** 2 * 9 * (32 * 32 - 16 * 32)
    say("batch %d  size %d  %s detector forward  (t) tiny %.3f ms  (k) darknet %.3f ms  (t)/(k) %.3f;  algorithmic FLOPs per "
        "pass (t) %.3e as run, %.3e at the file's widths  (k) %.3e  (t)/(k) %.3f" %
        (n, size, args.dtype, med["t"], med["k"], med["t"] / med["k"], ft, ft_file, fk, ft / fk))
    a = layer_ms(tiny.stem, lambda: tiny.forward(images), args.inner)
    say("  padding, forward: stack layer 0 %.4f ms, layer 1 %.4f ms, the stem's six layers %.4f ms (per-layer events, "
        "serialised launches); at most half of layers 0 + 1, %.4f ms, is what native 16-wide kernels could save: %.1f %% of (t)"
        % (a[0].sum(), a[1].sum(), a.sum(), 0.5 * (a[0].sum() + a[1].sum()),
           100 * 0.5 * (a[0].sum() + a[1].sum()) / med["t"]))
    del tiny, dark
    # ---- train step
    n = args.step_batch
    images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
    truth = np.zeros((n, 30, 5), np.float32)
    for i in range(n):
        for j in range(2):
            w, h = rng.uniform(0.1, 0.5, 2) * size
            truth[i, j] = (rng.uniform(0.3, 0.7) * size, rng.uniform(0.3, 0.7) * size, w, h, rng.integers(0, 20))
    truth = torch.from_numpy(truth).cuda()
    ntruth = torch.full((n,), 2, dtype=torch.int32, device="cuda")
    kw = dict(dtype=args.dtype, width_div=args.width_div, solver=Solver())
    tiny = yolov2.YOLOv2DarknetTrainer(n, size, anchors=yolov2.ANCHORS_TINY_VOC, topology="tiny", **kw)
    dark = yolov2.YOLOv2DarknetTrainer(n, size, **kw)
    med = medians([("T", lambda: tiny.step(images, truth=truth, ntruth=ntruth)),
                   ("K", lambda: dark.step(images, truth=truth, ntruth=ntruth))], inner=args.inner, warm=3)
    ft, fk = tiny.flops_per_step(size), dark.flops_per_step(size)
    say("batch %d  size %d  %s train step, box labels, DarknetSGD  (T) tiny %.3f ms  (K) darknet %.3f ms  (T)/(K) %.3f;  "
        "algorithmic FLOPs per step (T) %.3e  (K) %.3e  (T)/(K) %.3f" %
        (n, size, args.dtype, med["T"], med["K"], med["T"] / med["K"], ft, fk, ft / fk))
    a = layer_ms(tiny.networks()[0], lambda: tiny.step(images, truth=truth, ntruth=ntruth), args.inner)
    say("  padding, train step: stack layer 0 %.4f ms, layer 1 %.4f ms, the stem's six layers %.4f ms (per-layer events, "
        "serialised launches); at most half of layers 0 + 1, %.4f ms, is what native 16-wide kernels could save: %.1f %% of (T)"
        % (a[0].sum(), a[1].sum(), a.sum(), 0.5 * (a[0].sum() + a[1].sum()),
           100 * 0.5 * (a[0].sum() + a[1].sum()) / med["T"]))
    for name, tr in (("T", tiny), ("K", dark)):
        fin = all(bool(torch.isfinite(net.params).all()) for net in tr.networks())
        say("  (%s) parameters finite after the run: %s; steps skipped by the overflow guard: %d" %
            (name, fin, tr.opts[0].scaler.state()[2] if tr.opts[0].scaler is not None else 0))
    p0, p1 = tiny.networks()[0].export_params()[:2]
    say("  (T) padded entries still zero: %s" % (not p0["W"][..., 16:].any() and not p1["W"][:, :, 16:].any()))
    return finish(args, lines)


def finish(args, lines):
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
