"""What the device-resident VOC batches cost (img_dataset/device_voc.py, csrc/data.hip), on a devkit generated from a
seed (JPEGs of VOC-like shapes, 333..500 x 375..500, random annotations):

  kernels   per size of trainer.MULTI_SCALE_SIZES, batch 64: microseconds of the resize launch and of the label launch
            (HIP events around each launch, median), and the resize kernel's bytes per second = (the source rows the
            batch reads once + the batch bytes written) / time, next to the 4.4 TB/s the fp32 batch-norm passes reach
  step      f16 detector train step at batch 64 fed from DeviceVOC.get(size) against the same step on a resident uint8
            batch of the same size, at 320, 416 and 608: blocks of steps alternate between the two, HIP events around
            every step, median over all blocks.  The fed step must be no slower than 1.04 x the resident one
  host      for the record: pascal_voc.get_u8() with a cold cache at the same three sizes (what the device path replaces)

    python scripts/bench_device_voc.py --out profiles/device_voc_batch.txt
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow")


def make_devkit(root, images, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    voc = os.path.join(root, "VOC2007")
    for d in ("JPEGImages", "Annotations", os.path.join("ImageSets", "Main")):
        os.makedirs(os.path.join(voc, d), exist_ok=True)
    names = []
    for k in range(images):
        name = "%06d" % (k + 1)
        h, w = int(rng.integers(333, 501)), int(rng.integers(375, 501))
        # smooth random content (JPEG of white noise is not what a photograph costs to decode)
        small = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
        Image.fromarray(small).resize((w, h), Image.BILINEAR).save(os.path.join(voc, "JPEGImages", name + ".jpg"), quality=90)
        objs = []
        for _ in range(int(rng.integers(1, 6))):
            x = np.sort(rng.integers(1, w + 1, 2))
            y = np.sort(rng.integers(1, h + 1, 2))
            objs.append("<object><name>%s</name><bndbox><xmin>%d</xmin><ymin>%d</ymin><xmax>%d</xmax><ymax>%d</ymax>"
                        "</bndbox></object>" % (CLASSES[int(rng.integers(0, len(CLASSES)))], x[0], y[0], x[1], y[1]))
        with open(os.path.join(voc, "Annotations", name + ".xml"), "w") as f:
            f.write("<annotation><size><width>%d</width><height>%d</height><depth>3</depth></size>%s</annotation>"
                    % (w, h, "".join(objs)))
        names.append(name)
    with open(os.path.join(voc, "ImageSets", "Main", "trainval.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return root


def event_us(fn, warmup, reps):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30, help="timed launches per kernel and size (median)")
    ap.add_argument("--step-sizes", default="320,416,608")
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import ctypes as C
    import torch
    from tensorflow_yolo2_amd import _lib, synthetic, trainer
    from tensorflow_yolo2_amd.img_dataset.device_voc import DeviceVOC
    from tensorflow_yolo2_amd.img_dataset.pascal_voc import pascal_voc
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    with tempfile.TemporaryDirectory() as tmp:
        kit = make_devkit(os.path.join(tmp, "VOCdevkit"), args.images, seed=0)
        t0 = time.perf_counter()
        ds = DeviceVOC("trainval", batch_size=args.batch, devkit_path=kit, flipped=True, seed=0)
        torch.cuda.synchronize()
        say("device_voc batch %d, %d images (%d entries with flips), pool %.1f MB, start-up %.2f s"
            % (args.batch, len(ds.entries), len(ds.gt_labels), ds.pool_bytes / 1e6, time.perf_counter() - t0))
        lib = _lib.load()
        table = ds.table.cpu().numpy()
        ptr = lambda t: C.c_void_p(t.data_ptr())
        say()
        say("kernels (median of %d launches, HIP events)" % args.reps)
        say("size  resize_us  labels_us  resize_MB_read+written  resize_TB/s  of_4.4_TB/s")
        for size in trainer.MULTI_SCALE_SIZES:
            images, labels, index = ds.buffers(size)
            entries = np.array([ds._next()['entry'] for _ in range(args.batch)], np.int32)
            index.copy_(torch.from_numpy(entries))
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            rs = lambda: _lib.check(lib.y2_resize_bilinear_u8_batch(ptr(ds.pool), ptr(ds.table), ptr(index), args.batch,
                                                                    size, size, ptr(images), stream))
            lb = lambda: _lib.check(lib.y2_encode_labels(ptr(ds.boxes), ptr(ds.counts), ptr(ds.table), ptr(index),
                                                         args.batch, ds.max_obj, size, size // 32, ds.num_class,
                                                         ptr(labels), stream))
            t_rs = statistics.median(event_us(rs, args.warmup, args.reps))
            t_lb = statistics.median(event_us(lb, args.warmup, args.reps))
            nbytes = int(sum(table[e, 1] * table[e, 3] for e in entries)) + images.numel()
            rate = nbytes / (t_rs * 1e-6) / 1e12
            say("%4d  %9.1f  %9.1f  %22.1f  %11.2f  %10.2f" % (size, t_rs, t_lb, nbytes / 1e6, rate, rate / 4.4))
        say()
        say("f16 train step, batch %d: fed from DeviceVOC.get(size) vs a resident uint8 batch (median of %d x %d steps "
            "per variant, alternating blocks, HIP events)" % (args.batch, args.blocks, args.steps))
        say("size  resident_ms  fed_ms  fed/resident")
        for size in [int(v) for v in args.step_sizes.split(",")]:
            tr = trainer.DetectorTrainer(args.batch, size, dtype="f16")
            S = size // 32
            res_i = torch.from_numpy(np.random.default_rng(size).integers(0, 256, (args.batch, size, size, 3),
                                                                          dtype=np.uint8)).cuda()
            res_l = torch.as_tensor(synthetic.det_labels(args.batch, size, S, 4321)).cuda()
            resident = lambda: tr.step(res_i, res_l)
            fed = lambda: tr.step(*ds.get(size))
            times = {"resident": [], "fed": []}
            for fn in (resident, fed):
                event_us(fn, args.warmup, 0)
            for _ in range(args.blocks):
                times["resident"] += event_us(resident, 1, args.steps)
                times["fed"] += event_us(fed, 1, args.steps)
            r, f = statistics.median(times["resident"]) / 1e3, statistics.median(times["fed"]) / 1e3
            say("%4d  %11.3f  %6.3f  %12.4f" % (size, r, f, f / r))
            del tr, res_i, res_l, resident, fed
            torch.cuda.empty_cache()
        if not args.skip_host:
            say()
            say("host pascal_voc.get_u8(), batch %d, cold cache (one batch, wall clock)" % args.batch)
            say("size  seconds")
            for size in [int(v) for v in args.step_sizes.split(",")]:
                host = pascal_voc("trainval", batch_size=args.batch, devkit_path=kit, image_size=size, flipped=True,
                                  seed=0, cache_images=False)
                t0 = time.perf_counter()
                host.get_u8()
                say("%4d  %7.2f" % (size, time.perf_counter() - t0))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
