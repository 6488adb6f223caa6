"""What the region statistics cost, and what a full-width cfg model's forward pass takes:

  (s) statistics  y2_yolov2_region_stats (a workgroup per image + the finalize)
  (l) list loss   y2_yolov2_loss_boxes on the same tensors, with its gradient, as the train step runs it
  (n) list loss   ... without the gradient
  (l') list loss  (l) again: the spread of one leg against itself, in the same blocks
      at batch 64, heads of 416 x 416 (S 13, 845 slots per image) and 608 x 608 (S 19, 1805), 5 anchors, 20 classes,
      30 truths per image, area weight and prior on
  (t) step        the f16 train step of the "darknet" graph (YOLOv2DarknetTrainer, full width) on a fixed batch and box
                  list: step(truth=, ntruth=) against step(truth=, ntruth=, stats=)
  (f) forward     YOLOv2Detector.from_cfg of a full-width yolov2.cfg (80 classes) beside the "darknet" VOC graph, batch
                  32, f16, 416 and 608 -- for information, no claim

HIP events around blocks of --inner calls after a warm-up of every leg; the legs alternate inside every repetition and the
median over --reps repetitions is reported.  The claim under test: (s) costs no more than (l) at the same shape, within
the +-4 % box-to-box spread the README states.  The step's difference is reported as measured.

    python scripts/bench_region_stats.py --out profiles/region_stats.txt
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
    ap.add_argument("--sizes", default="416,608")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=400)
    ap.add_argument("--step-inner", type=int, default=5)
    ap.add_argument("--step-size", type=int, default=416)
    ap.add_argument("--forward-batch", type=int, default=32)
    ap.add_argument("--forward-inner", type=int, default=10)
    ap.add_argument("--cfg", default=os.path.join(ROOT, "tests", "golden", "cfg", "yolov2.cfg"))
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import _lib, engine as E
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _lib.load()
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
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                us[name].append(block_us(fn, inner))
        return {k: statistics.median(v) for k, v in us.items()}

    n, B, Cn, T = args.batch, 5, 20, 30
    ptr, stream = E._ptr, E._stream
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)

    def box_list(batch, size):
        full = np.zeros((batch, T, 5), np.float32)
        full[..., 0:2] = rng.uniform(1, size - 1, (batch, T, 2))
        full[..., 2:4] = rng.uniform(0.05 * size, 0.6 * size, (batch, T, 2))
        full[..., 4] = rng.integers(0, Cn, (batch, T))
        return torch.from_numpy(full).cuda(), torch.full((batch,), T, dtype=torch.int32, device="cuda")

    say("Region statistics beside the box-list loss, batch %d, %d anchors, %d classes, %d truths per image; HIP events, median "
        "of %d alternating blocks of %d calls, microseconds per call (both launches of each: kernel + finalize)"
        % (n, B, Cn, T, args.reps, args.inner))
    say("size  slots/img  (s) statistics  (l) loss + gradient  (n) loss alone  (l') loss + gradient again  (s)/(l)  (l')/(l)")
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        net = torch.from_numpy((rng.standard_normal((n, S, S, B, 5 + Cn)) * 0.7).astype(np.float32)).cuda()
        truth, ntruth = box_list(n, size)
        loss, dnet, stats = torch.empty(5, device="cuda"), torch.empty_like(net), torch.empty(6, device="cuda")
        ws = torch.empty(lib.y2_yolov2_loss_boxes_workspace_bytes(n, S, B) + 4096, dtype=torch.uint8, device="cuda")
        ws_s = torch.empty(lib.y2_yolov2_region_stats_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        sc = (C.c_float * 7)(1.0, 5.0, 1.0, 1.0, 0.6, 1.0, 0.01)

        def region_stats():
            E.check(lib.y2_yolov2_region_stats(ptr(net), ptr(truth), ptr(ntruth), ptr(anchors), n, S, B, Cn, T, float(size),
                                               ptr(stats), ptr(ws_s), stream()))

        def list_loss(grad=dnet):
            E.check(lib.y2_yolov2_loss_boxes(ptr(net), ptr(truth), ptr(ntruth), ptr(anchors), n, S, B, Cn, T, float(size),
                                             sc, ptr(loss), ptr(grad), ptr(ws), stream()))

        med = medians([("s", region_stats), ("l", list_loss), ("n", lambda: list_loss(None)), ("l2", list_loss)], args.inner)
        say("%4d  %9d  %14.2f  %19.2f  %14.2f  %26.2f  %7.3f  %8.3f" % (size, S * S * B, med["s"], med["l"], med["n"], med["l2"],
                                                                      med["s"] / med["l"], med["l2"] / med["l"]))
    if not args.no_step:
        size = args.step_size
        say()
        say("f16 train step of the \"darknet\" graph (full width, batch %d, size %d, box list of %d truths, Adam): milliseconds "
            "per step, median of %d alternating blocks of %d steps" % (n, size, T, args.reps, args.step_inner))
        say("without stats  with stats  difference (us)  again without  again - without (us)")
        images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
        truth, ntruth = box_list(n, size)
        stats = torch.empty(6, device="cuda")
        plain = yolov2.YOLOv2DarknetTrainer(n, size, dtype="f16", seed=0)
        with_stats = yolov2.YOLOv2DarknetTrainer(n, size, dtype="f16", seed=0)
        med = medians([("p", lambda: plain.step(images, truth=truth, ntruth=ntruth)),
                       ("s", lambda: with_stats.step(images, truth=truth, ntruth=ntruth, stats=stats)),
                       ("p2", lambda: plain.step(images, truth=truth, ntruth=ntruth))], args.step_inner)
        say("%13.3f  %10.3f  %15.1f  %13.3f  %20.1f" % (med["p"] / 1e3, med["s"] / 1e3, med["s"] - med["p"], med["p2"] / 1e3,
                                                        med["p2"] - med["p"]))
        del plain, with_stats
        torch.cuda.empty_cache()
    if not args.no_forward:
        nb = args.forward_batch
        say()
        say("forward pass, batch %d, f16, uint8 input: the model of %s (YOLOv2Detector.from_cfg) beside the \"darknet\" VOC "
            "graph; milliseconds, median of %d alternating blocks of %d passes (information only)"
            % (nb, os.path.relpath(args.cfg, ROOT), args.reps, args.forward_inner))
        say("size  cfg model  \"darknet\" VOC graph")
        for size in [int(v) for v in args.sizes.split(",")]:
            images = torch.from_numpy(rng.integers(0, 256, (nb, size, size, 3), dtype=np.uint8)).cuda()
            coco = yolov2.YOLOv2Detector.from_cfg(args.cfg, nb, size, dtype="f16")
            voc = yolov2.YOLOv2Detector(nb, size, dtype="f16", topology="darknet")
            med = medians([("c", lambda: coco.forward(images)), ("v", lambda: voc.forward(images))], args.forward_inner)
            say("%4d  %9.3f  %19.3f" % (size, med["c"] / 1e3, med["v"] / 1e3))
            del coco, voc
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
