"""What the graph of yolov2-voc.cfg costs beside the paper's (yolo2_nets/yolov2.py: YOLOv2Detector(topology="darknet");
csrc/ext.hip: y2_passthrough_concat_darknet, y2_u8_bgr_to_f32_rgb), batch 32, one MI355X:

  (s) / (d)   y2_passthrough_concat (space-to-depth, two launches) / y2_passthrough_concat_darknet (Darknet's scramble,
              one launch) at Cf = 64, Cc = 1024, S = 13 and 19: the same bytes out, so the ratio prices the gather
  (u)         y2_u8_bgr_to_f32_rgb on a batch of the input size
  (p) / (k)   YOLOv2Detector.forward on a uint8 batch, paper / darknet topology, --dtype (f16), 416 x 416 and 608 x 608
  f16 / f32   the darknet topology's f16 head against its f32 head on the same random weights and batch: a figure

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  The claim under test: (k) is the faster graph, by about the saved channels of the 3x3 layer
behind the passthrough (3072 -> 1280 input channels: 5.6 GFLOP per 416 x 416 image).

    python scripts/bench_darknet_yolov2.py --out profiles/darknet_yolov2.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--sizes", default="416,608")
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E
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

    def medians(legs, inner=None):
        inner = inner or args.inner
        for _name, fn in legs:                                   # warm-up: kernel loads, filter packs
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                ms[name].append(block_ms(fn, inner))
        return {k: statistics.median(v) for k, v in ms.items()}

    n = args.batch
    rng = np.random.default_rng(0)
    say("YOLOv2, Darknet's graph beside the paper's, batch %d, width_div %d; HIP events, median of %d alternating blocks of "
        "%d calls (%d for the single launches), milliseconds per call" % (n, args.width_div, args.reps, args.inner,
                                                                           10 * args.inner))
    lib = E._lib.load()
    cf, cc = 64, 1024
    for S in (13, 19):
        fine = torch.from_numpy(rng.standard_normal((n, 2 * S, 2 * S, cf)).astype(np.float32)).cuda()
        coarse = torch.from_numpy(rng.standard_normal((n, S, S, cc)).astype(np.float32)).cuda()
        out = torch.empty((n, S, S, 4 * cf + cc), dtype=torch.float32, device="cuda")

        def plain():
            E.check(lib.y2_passthrough_concat(E._ptr(fine), E._ptr(coarse), E._ptr(out), n, S, S, cf, cc, E._stream()))

        def darknet():
            E.passthrough_concat_darknet(fine, coarse, out=out)

        med = medians([("s", plain), ("d", darknet)], inner=10 * args.inner)       # launches of tens of microseconds
        moved = (fine.numel() + coarse.numel() + out.numel()) * 4
        say("concat  S %2d  Cf %d  Cc %d  (s) space-to-depth %.4f  (d) darknet %.4f  (d)/(s) %.3f  (d) moves %.2f TB/s" %
            (S, cf, cc, med["s"], med["d"], med["d"] / med["s"], moved / med["d"] / 1e9))
    for size in [int(v) for v in args.sizes.split(",")]:
        images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
        rgb = torch.empty((n, size, size, 3), dtype=torch.float32, device="cuda")
        u_ms = medians([("u", lambda: E.u8_to_darknet_input(images, out=rgb))], inner=10 * args.inner)["u"]
        say("size %4d  (u) input conversion %.4f" % (size, u_ms))
        if args.no_forward:
            continue
        paper = yolov2.YOLOv2Detector(n, size, dtype=args.dtype, width_div=args.width_div)
        dark = yolov2.YOLOv2Detector(n, size, dtype=args.dtype, width_div=args.width_div, topology="darknet")
        # parameters of a trained network's scale (the initial ones, filters of deviation 0.1 behind moving statistics
        # 0 / 1, grow ten-fold per layer and leave the half-precision range): filters He-scaled, variances in [0.5, 2]
        for net in dark.networks():
            layers = net.export_params()
            for p in layers:
                k, _, c, co = p["W"].shape
                p.update(W=rng.normal(0, np.sqrt(2.0 / (c * k * k)), p["W"].shape).astype(np.float32),
                         b=np.zeros(co, np.float32), gamma=rng.uniform(0.8, 1.2, co).astype(np.float32),
                         beta=rng.normal(0, 0.2, co).astype(np.float32),
                         moving_mean=rng.normal(0, 0.2, co).astype(np.float32),
                         moving_var=rng.uniform(0.5, 2.0, co).astype(np.float32))
            net.load_params(layers)
        med = medians([("p", lambda: paper.forward(images)), ("k", lambda: dark.forward(images))])
        say("size %4d  %s forward  (p) paper %.4f  (k) darknet %.4f  (k)/(p) %.3f  (p)-(k) %.4f" %
            (size, args.dtype, med["p"], med["k"], med["k"] / med["p"], med["p"] - med["k"]))
        del paper
        # the darknet topology's half-precision head against its f32 head: the same parameters, the same batch
        full = yolov2.YOLOv2Detector(n, size, dtype="f32", width_div=args.width_div, topology="darknet")
        for a, b in zip(dark.networks(), full.networks()):
            b.load_params(a.export_params())
        g16 = dark.forward(images).float().cpu().numpy().copy()
        g32 = full.forward(images).cpu().numpy()
        say("size %4d  darknet topology, %s head against f32 (random parameters): max |d| / max |ref| %.3e, finite %s" %
            (size, args.dtype, np.abs(g16 - g32).max() / np.abs(g32).max(), bool(np.isfinite(g16).all())))
        del dark, full
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
