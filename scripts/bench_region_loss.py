"""What the box-list labels of the anchor model cost, batch 64, heads of 416 x 416 (845 slots per image) and 608 x 608
(1805), 5 anchors, 20 classes:

  (g) grid loss   y2_yolov2_loss on the label grid (one workgroup per image) -- from --parent-lib when given (a
                  libyolo2_hip.so built from the parent commit, loaded next to this tree's), else this tree's library
  (l) list loss   y2_yolov2_loss_boxes on the box list of the SAME collision-free objects (grid of 256-slot workgroups)
  (L) list loss   ... with 30 truths per image, the area weight and the prior on
  (e) encoder     y2_encode_box_list alone, 64 images of the seeded devkit of scripts/bench_device_voc.py, plain and windowed
  (s) step        the f16 train step (YOLOv2Trainer, full width) fed by DeviceVOC.get(size): label grid against
                  max_boxes = 30 + step(truth=, ntruth=)

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  The claims under test: (l) is no slower than (g); the list path adds no more to the step than
its two launches.

    python scripts/bench_region_loss.py [--parent-lib PATH] --out profiles/region_loss.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sizes", default="416,608")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step-inner", type=int, default=5)
    ap.add_argument("--images", type=int, default=128, help="JPEGs of the seeded devkit")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--parent-lib", default=None, help="libyolo2_hip.so of the parent commit: its grid loss is the baseline")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from bench_device_voc import make_devkit
    from tensorflow_yolo2_amd import _lib, engine as E, synthetic
    from tensorflow_yolo2_amd.img_dataset.augment import Augment
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.utils import region_loss as RL
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _lib.load()
    base, base_name = lib, "this tree's library"
    if args.parent_lib:
        base = C.CDLL(os.path.abspath(args.parent_lib))
        assert not hasattr(base, "y2_yolov2_loss_boxes"), "--parent-lib exports the new kernels: not the parent's build"
        name, (res, argtypes) = "y2_yolov2_loss", _lib.SIGNATURES["y2_yolov2_loss"]
        getattr(base, name).restype, getattr(base, name).argtypes = res, argtypes
        base_name = "the parent commit's build"
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

    n, B, Cn, T = args.batch, 5, 20, 30
    ptr, stream = E._ptr, E._stream
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    say("Region loss on box lists, batch %d, %d anchors, %d classes; HIP events, median of %d alternating blocks, "
        "microseconds per call (both launches of a loss: kernel + finalize); grid loss from %s" % (n, B, Cn, args.reps, base_name))
    say("size  slots/img  objects/img  (g) grid loss  (l) list loss, same objects  (L) list loss, 30 truths + area + prior  (l)/(g)")
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        net = torch.from_numpy((rng.standard_normal((n, S, S, B, 5 + Cn)) * 0.7).astype(np.float32)).cuda()
        lab = synthetic.det_labels(n, size, S, 5)
        truth_np, ntruth_np = RL.grid_to_box_list(lab, T)
        labels, truth, ntruth = (torch.from_numpy(a).cuda() for a in (lab, truth_np, ntruth_np))
        full = np.zeros((n, T, 5), np.float32)
        full[..., 0:2] = rng.uniform(1, size - 1, (n, T, 2))
        full[..., 2:4] = rng.uniform(0.05 * size, 0.6 * size, (n, T, 2))
        full[..., 4] = rng.integers(0, Cn, (n, T))
        truth30 = torch.from_numpy(full).cuda()
        ntruth30 = torch.full((n,), T, dtype=torch.int32, device="cuda")
        loss, dnet = torch.empty(5, device="cuda"), torch.empty_like(net)
        ws = torch.empty(lib.y2_yolov2_loss_boxes_workspace_bytes(n, S, B) + 4096, dtype=torch.uint8, device="cuda")
        sc30 = (C.c_float * 7)(1.0, 5.0, 1.0, 1.0, 0.6, 1.0, 0.01)

        def grid_loss():
            E.check(base.y2_yolov2_loss(ptr(net), ptr(labels), ptr(anchors), n, S, B, Cn, float(size), None, ptr(loss),
                                        ptr(dnet), ptr(ws), stream()))

        def list_loss():
            E.check(lib.y2_yolov2_loss_boxes(ptr(net), ptr(truth), ptr(ntruth), ptr(anchors), n, S, B, Cn, T, float(size),
                                             None, ptr(loss), ptr(dnet), ptr(ws), stream()))

        def list_loss30():
            E.check(lib.y2_yolov2_loss_boxes(ptr(net), ptr(truth30), ptr(ntruth30), ptr(anchors), n, S, B, Cn, T,
                                             float(size), sc30, ptr(loss), ptr(dnet), ptr(ws), stream()))

        med = medians([("g", grid_loss), ("l", list_loss), ("L", list_loss30)], args.inner)
        say("%4d  %9d  %11.1f  %13.1f  %27.1f  %40.1f  %7.2f" % (size, S * S * B, float(ntruth_np.mean()), med["g"], med["l"],
                                                                   med["L"], med["l"] / med["g"]))
    with tempfile.TemporaryDirectory() as tmp:
        kit = make_devkit(os.path.join(tmp, "VOCdevkit"), args.images, seed=0)
        plain = DeviceVOC("trainval", batch_size=n, devkit_path=kit, seed=0)
        lists = DeviceVOC("trainval", batch_size=n, devkit_path=kit, seed=0, max_boxes=T)
        say()
        say("y2_encode_box_list alone, %d images of the seeded devkit (max_obj %d), max_boxes %d: microseconds per launch"
            % (n, lists.max_obj, T))
        say("size  identity rows  windowed rows  y2_encode_labels (the grid, for scale)")
        for size in [int(v) for v in args.sizes.split(",")]:
            index = torch.from_numpy(rng.integers(0, len(lists.entries), n).astype(np.int32)).cuda()
            aug, arng = Augment(), np.random.default_rng(1)
            rows = np.stack([aug.draw(arng, *lists.entries[int(e)]['shape']) for e in index.cpu().numpy()])
            params = torch.from_numpy(rows).cuda()
            truth = torch.empty((n, T, 5), dtype=torch.float32, device="cuda")
            ntruth = torch.empty(n, dtype=torch.int32, device="cuda")
            grid = torch.empty((n, size // 32, size // 32, 25), dtype=torch.float32, device="cuda")

            def enc(p):
                return lambda: E.check(lib.y2_encode_box_list(ptr(lists.boxes), ptr(lists.counts), ptr(lists.table),
                                                              ptr(index), p, n, lists.max_obj, size, T, ptr(truth),
                                                              ptr(ntruth), stream()))

            def enc_grid():
                E.check(lib.y2_encode_labels(ptr(lists.boxes), ptr(lists.counts), ptr(lists.table), ptr(index), n,
                                             lists.max_obj, size, size // 32, 20, ptr(grid), stream()))

            med = medians([("i", enc(None)), ("w", enc(ptr(params))), ("g", enc_grid)], args.inner)
            say("%4d  %13.1f  %13.1f  %13.1f" % (size, med["i"], med["w"], med["g"]))
        if not args.no_step:
            say()
            say("f16 train step (full width, batch %d) fed by DeviceVOC.get(size): milliseconds per step, get() included" % n)
            say("size  label grid  box list (max_boxes %d)  difference (us)" % T)
            for size in [int(v) for v in args.sizes.split(",")]:
                tr_grid = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=0)
                tr_list = yolov2.YOLOv2Trainer(n, size, dtype="f16", seed=0)

                def step_grid():
                    images, labels = plain.get(size)
                    tr_grid.step(images, labels)

                def step_list():
                    images, _labels, truth, ntruth = lists.get(size)
                    tr_list.step(images, truth=truth, ntruth=ntruth)

                med = medians([("g", step_grid), ("l", step_list)], args.step_inner)
                say("%4d  %10.3f  %23.3f  %15.1f" % (size, med["g"] / 1e3, med["l"] / 1e3, med["l"] - med["g"]))
                del tr_grid, tr_list
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
