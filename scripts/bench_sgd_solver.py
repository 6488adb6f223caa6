"""What Darknet's SGD solver costs beside Adam on the YOLOv2 anchor model (full width, guarded f16):

  (a) Adam        y2_adam_step_packed of one stack: update + filter re-pack, 28 B per parameter in and out + the packs
  (s) SGD         y2_sgd_step_packed on the SAME context, parameters and gradients: 16 B per parameter + the packs
  (f) SGD, flat   y2_sgd_step: the update alone (the next forward then re-packs), for scale
  (t) step        YOLOv2Trainer.step at --size, batch --batch, under both optimizers

for the three stacks (stem, 13x13 stack, head) and their sum.  HIP events around blocks of --inner calls; the legs
alternate inside every repetition and the median over --reps repetitions is reported.  Every leg runs the control block's
advance kernel too, as a train step does.  The claim under test: (s) is no slower than (a) -- on an HBM-bound launch
roughly (16 + 4) / (28 + 4) of it.

    python scripts/bench_sgd_solver.py --out profiles/sgd_solver.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-inner", type=int, default=5)
    ap.add_argument("--width-div", type=int, default=1)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.utils.solver import Solver
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
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

    def medians(legs, inner):
        for _name, fn in legs:
            fn()
        torch.cuda.synchronize()
        us = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                us[name].append(block_us(fn, inner))
        return {k: statistics.median(v) for k, v in us.items()}

    n, size = args.batch, args.size
    sv = Solver(burn_in=0)                      # the rate of a trained run; the schedule kernel runs all the same
    say("Darknet's SGD step against the Adam step, YOLOv2 stacks (width / %d), guarded f16; HIP events, median of %d "
        "alternating blocks of %d calls, microseconds per call" % (args.width_div, args.reps, args.inner))
    say("stack  parameters  (a) Adam packed  (s) SGD packed  (f) SGD flat  (s)/(a)  (s) GB/s of 20 B/param")
    S = size // 32
    specs = yolov2.yolov2_specs(20, 5, args.width_div)
    rng = np.random.default_rng(0)
    total = {"a": 0.0, "s": 0.0, "f": 0.0}
    for name, spec, h in zip(("stem", "deep", "head"), specs, (size, S, S)):
        net = E.Network(spec, n, h, h, dtype="f16", training=True)
        net.init_params(1)
        net.grads.copy_(torch.from_numpy((rng.standard_normal(net.n_params) * 1e-3).astype(np.float32)))
        adam = E.AdamOptimizer(net)
        sgd = E.DarknetSGD(net, sv)
        flat = E.DarknetSGD(net, sv, fused_pack=False)
        flat.accum = sgd.accum                  # the same slot: one working set beside Adam's two
        for opt in (adam, sgd, flat):
            opt.scaler.scan(net)                # a clean flag; the legs do not scan (the step's scan is not the solver's)
        ptr, stream = E._ptr, E._stream

        def leg_adam():
            E.check(net.lib.y2_adam_step_packed(net.h, ptr(adam.m), ptr(adam.v), ptr(adam.scaler.ctrl), 1, adam.lr, adam.b1,
                                                adam.b2, adam.eps, 1.0, stream()))

        def leg_sgd():
            E.check(net.lib.y2_sgd_step_packed(net.h, ptr(sgd.accum), ptr(sgd.scaler.ctrl), 1, C.byref(sgd._record), 1.0,
                                               stream()))

        def leg_flat():
            E.check(net.lib.y2_sgd_step(net.h, ptr(flat.accum), ptr(flat.scaler.ctrl), 1, C.byref(flat._record), 1.0,
                                        stream()))

        med = medians([("a", leg_adam), ("s", leg_sgd), ("f", leg_flat)], args.inner)
        for k in total:
            total[k] += med[k]
        say("%-5s  %10d  %15.1f  %14.1f  %12.1f  %7.2f  %10.0f" % (name, net.n_params, med["a"], med["s"], med["f"],
                                                                   med["s"] / med["a"], 20.0 * net.n_params / med["s"] / 1e3))
        assert torch.isfinite(net.params).all()
        del net, adam, sgd, flat
        torch.cuda.empty_cache()
    say("%-5s  %10s  %15.1f  %14.1f  %12.1f  %7.2f" % ("sum", "", total["a"], total["s"], total["f"], total["s"] / total["a"]))
    if not args.no_step:
        say()
        say("YOLOv2Trainer.step, f16, batch %d at %d x %d, label grid: milliseconds per step" % (n, size, size))
        say("(A) Adam  (S) Darknet SGD  (S)/(A)")
        x = torch.as_tensor(synthetic.images(n, size, 1)).cuda()
        lab = np.zeros((n, S, S, 25), np.float32)
        lab[:, S // 2, S // 2, 0] = 1
        lab[:, S // 2, S // 2, 1:5] = (size / 2.0, size / 2.0, size / 4.0, size / 3.0)
        lab[:, S // 2, S // 2, 5 + 7] = 1
        lab = torch.as_tensor(lab).cuda()
        tr_a = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=0, width_div=args.width_div)
        tr_s = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=0, width_div=args.width_div, solver=sv)
        med = medians([("A", lambda: tr_a.step(x, lab)), ("S", lambda: tr_s.step(x, lab))], args.step_inner)
        say("%8.3f  %15.3f  %7.3f" % (med["A"] / 1e3, med["S"] / 1e3, med["S"] / med["A"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
