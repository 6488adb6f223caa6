"""What the augmented device-resident VOC batches cost (img_dataset/device_voc.py with an Augment, csrc/augment.hip), on
the seeded devkit of scripts/bench_device_voc.py (256 JPEGs of VOC-like shapes):

  kernels   per size of trainer.MULTI_SCALE_SIZES, batch 64: microseconds of y2_augment_u8_batch (rows drawn at the
            default jitter 0.3, hue 0.1, saturation 1.5, exposure 1.5) and y2_encode_labels_window next to the plain
            y2_resize_bilinear_u8_batch and y2_encode_labels on the SAME entries -- from --parent-lib when given (a
            libyolo2_hip.so built from the parent commit, loaded next to this tree's), else from this tree's library --
            HIP events around each launch, median; the four launches alternate inside every repetition
  step      f16 detector train step at batch 64 fed from augmented get(size) against fed from plain get(size), at 320,
            416 and 608: blocks of steps alternate between the two, HIP events around every step, median over all blocks

    python scripts/bench_device_voc_augment.py [--parent-lib PATH] --out profiles/device_voc_augment.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_device_voc import event_us, make_devkit  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30, help="timed launches per kernel and size (median)")
    ap.add_argument("--step-sizes", default="320,416,608")
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libyolo2_hip.so of the parent commit: its plain kernels are the baseline")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import _lib, trainer
    from tensorflow_yolo2_amd.img_dataset.augment import Augment
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    lib = _lib.load()
    base, base_name = lib, "this build"
    if args.parent_lib:
        base = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("y2_resize_bilinear_u8_batch", "y2_encode_labels"):
            getattr(base, name).restype, getattr(base, name).argtypes = _lib.SIGNATURES[name]
        assert not hasattr(base, "y2_augment_u8_batch"), "--parent-lib exports the new kernels: not the parent's build"
        base_name = "the parent commit's build"
    with tempfile.TemporaryDirectory() as tmp:
        kit = make_devkit(os.path.join(tmp, "VOCdevkit"), args.images, seed=0)
        t0 = time.perf_counter()
        plain = DeviceVOC("trainval", batch_size=args.batch, devkit_path=kit, flipped=True, seed=0)
        ds = DeviceVOC("trainval", batch_size=args.batch, devkit_path=kit, flipped=True, seed=0, augment=Augment())
        torch.cuda.synchronize()
        say("device_voc augmented, batch %d, %d images (%d entries with flips), pool %.1f MB, two pools, start-up %.2f s"
            % (args.batch, len(ds.entries), len(ds.gt_labels), ds.pool_bytes / 1e6, time.perf_counter() - t0))
        say("augmentation %r; plain kernels from %s" % (ds.augment, base_name))
        table = ds.table.cpu().numpy()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        say()
        say("kernels (median of %d launches each, HIP events, the four launches alternate)" % args.reps)
        say("size  resize_us  augment_us  augment/resize  labels_us  labels_window_us  MB_read+written  augment_TB/s")
        for size in trainer.MULTI_SCALE_SIZES:
            images, labels, index = ds.buffers(size)
            entries = np.array([ds._next()['entry'] for _ in range(args.batch)], np.int32)
            rows = np.array([ds.augment.draw(ds.aug_rng, table[e, 1], table[e, 2]) for e in entries])
            index.copy_(torch.from_numpy(entries))
            params = torch.from_numpy(rows).cuda()
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            calls = {
                "resize": lambda: _lib.check(base.y2_resize_bilinear_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), args.batch, size, size, ptr(images), stream)),
                "augment": lambda: _lib.check(lib.y2_augment_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), ptr(params), args.batch, size, size, ds.augment.fill,
                    ptr(images), stream)),
                "labels": lambda: _lib.check(base.y2_encode_labels(
                    ptr(ds.boxes), ptr(ds.counts), ptr(ds.table), ptr(index), args.batch, ds.max_obj, size, size // 32,
                    ds.num_class, ptr(labels), stream)),
                "window": lambda: _lib.check(lib.y2_encode_labels_window(
                    ptr(ds.boxes), ptr(ds.counts), ptr(ds.table), ptr(index), ptr(params), args.batch, ds.max_obj, size,
                    size // 32, ds.num_class, ptr(labels), stream)),
            }
            times = {k: [] for k in calls}
            for fn in calls.values():
                event_us(fn, args.warmup, 0)
            for _ in range(args.reps):
                for k, fn in calls.items():
                    times[k] += event_us(fn, 0, 1)
            t = {k: statistics.median(v) for k, v in times.items()}
            # the source rows the windows touch (clipped to the image) + the batch bytes written
            nbytes = images.numel()
            for e, r in zip(entries, rows):
                lo, hi = max(int(r[1]), 0), min(int(r[1] + r[3]), int(table[e, 1]))
                nbytes += max(hi - lo, 0) * int(table[e, 3])
            say("%4d  %9.1f  %10.1f  %14.2f  %9.1f  %16.1f  %15.1f  %12.2f"
                % (size, t["resize"], t["augment"], t["augment"] / t["resize"], t["labels"], t["window"], nbytes / 1e6,
                   nbytes / (t["augment"] * 1e-6) / 1e12))
        t0 = time.perf_counter()
        for _ in range(20 * args.batch):
            ds.augment.draw(ds.aug_rng, 375, 500)
        say()
        say("host: drawing the %d parameter rows of one batch, inside get(): %.2f ms (wall clock, mean of 20 batches)"
            % (args.batch, (time.perf_counter() - t0) / 20 * 1e3))
        if not args.skip_steps:
            say()
            say("f16 train step, batch %d: fed from augmented get(size) vs plain get(size) (median of %d x %d steps per "
                "variant, alternating blocks, HIP events)" % (args.batch, args.blocks, args.steps))
            say("size  plain_ms  augmented_ms  difference_us  augmented/plain")
            for size in [int(v) for v in args.step_sizes.split(",")]:
                tr = trainer.DetectorTrainer(args.batch, size, dtype="f16")
                fed_plain = lambda: tr.step(*plain.get(size))
                fed_aug = lambda: tr.step(*ds.get(size))
                times = {"plain": [], "aug": []}
                for fn in (fed_plain, fed_aug):
                    event_us(fn, args.warmup, 0)
                for _ in range(args.blocks):
                    times["plain"] += event_us(fed_plain, 1, args.steps)
                    times["aug"] += event_us(fed_aug, 1, args.steps)
                p, a = statistics.median(times["plain"]) / 1e3, statistics.median(times["aug"]) / 1e3
                say("%4d  %8.3f  %12.3f  %13.1f  %15.4f" % (size, p, a, (a - p) * 1e3, a / p))
                del tr, fed_plain, fed_aug
                torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
