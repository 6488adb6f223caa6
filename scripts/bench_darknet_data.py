"""What Darknet's shuffle-then-cut costs in the training batches of a Darknet image list (img_dataset/device_boxes.py:
DeviceDarknet; csrc/augment.hip: y2_encode_box_list_draw), on the images of scripts/bench_device_voc.py's seeded devkit
(256 JPEGs of VOC-like shapes) as a Darknet list whose label files are COCO-like: three images in four hold 1 .. 12
objects, one in four 35 .. 60 (more than max_boxes = 30, so the draw has something to cut).

  get()     per batch of 64 at 416, augmented: get(size) with the draw off and with the draw on, from the SAME pool in the
            same process -- the draw is switched per block -- HIP events around every call, median over all blocks.  The
            draw-off figure is the parent commit's kernels: the baseline
  kernels   y2_encode_box_list and y2_encode_box_list_draw (with keys, and with keys = NULL) alone on one batch's index and
            parameter rows, HIP events around each launch, median; the launches alternate inside every repetition

    python scripts/bench_darknet_data.py --out profiles/darknet_data.txt
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


def make_list(kit, classes, seed):
    """the devkit's JPEGs as a Darknet list with label files of their own (labels/ beside JPEGImages/) -> the list path"""
    from tensorflow_yolo2_amd.utils import darknet_data
    rng = np.random.default_rng(seed)
    directory = os.path.join(kit, "VOC2007", "JPEGImages")
    paths = [os.path.join(directory, n) for n in sorted(os.listdir(directory))]
    for p in paths:
        n = int(rng.integers(35, 61)) if rng.integers(0, 4) == 0 else int(rng.integers(1, 13))
        rows = []
        for _ in range(n):
            w, h = rng.uniform(0.02, 0.4), rng.uniform(0.02, 0.4)
            rows.append((int(rng.integers(0, classes)), rng.uniform(w / 2, 1 - w / 2), rng.uniform(h / 2, 1 - h / 2), w, h))
        darknet_data.write_labels(darknet_data.label_path(p), rows)
    lst = os.path.join(kit, "train.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    return lst


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--max-boxes", type=int, default=30)
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--calls", type=int, default=20, help="timed get() calls per block")
    ap.add_argument("--reps", type=int, default=50, help="timed launches per kernel (median)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import _lib
    from tensorflow_yolo2_amd.img_dataset.augment import Augment
    from tensorflow_yolo2_amd.img_dataset.device_boxes import DeviceDarknet
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    lib = _lib.load()
    size, B, T = args.size, args.batch, args.max_boxes
    with tempfile.TemporaryDirectory() as tmp:
        kit = make_devkit(os.path.join(tmp, "VOCdevkit"), args.images, seed=0)
        lst = make_list(kit, 80, seed=1)
        t0 = time.perf_counter()
        ds = DeviceDarknet(lst, 80, batch_size=B, seed=0, augment=Augment(), max_boxes=T, draw=True)
        torch.cuda.synchronize()
        counts = ds.counts.cpu().numpy()
        say("darknet list, batch %d at %d, %d images, pool %.1f MB, max_obj %d, %d images with more than max_boxes = %d "
            "objects, start-up %.2f s" % (B, size, len(ds.entries), ds.pool_bytes / 1e6, ds.max_obj, int((counts > T).sum()),
                                          T, time.perf_counter() - t0))
        say()
        say("get(%d), augmented, draw off vs on from the same pool (median of %d x %d calls per variant, alternating "
            "blocks, HIP events)" % (size, args.blocks, args.calls))

        def get_with(draw):
            def fn():
                ds.draw = draw
                ds.get(size)
            return fn
        times = {False: [], True: []}
        for draw in (False, True):
            event_us(get_with(draw), args.warmup, 0)
        for _ in range(args.blocks):
            for draw in (False, True):
                times[draw] += event_us(get_with(draw), 1, args.calls)
        off, on = statistics.median(times[False]), statistics.median(times[True])
        say("draw_off_us  draw_on_us  difference_us  on/off")
        say("%11.1f  %10.1f  %13.1f  %6.4f" % (off, on, on - off, on / off))
        ds.draw = True
        from tensorflow_yolo2_amd.img_dataset.augment import draw_key
        from tensorflow_yolo2_amd.img_dataset.device_pool import upload_async
        t0 = time.perf_counter()
        for _ in range(200 * B):
            draw_key(ds.key_rng)
        host_keys = (time.perf_counter() - t0) / 200 * 1e6
        ds.get(size)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            upload_async(ds._keys[size], ds.last_keys.view(np.int32))
        torch.cuda.synchronize()
        host_upload = (time.perf_counter() - t0) / 200 * 1e6
        say("host, inside get() with the draw on: drawing the %d keys of a batch %.1f us, pinning and enqueueing their "
            "upload %.1f us (wall clock, mean of 200)" % (B, host_keys, host_upload))
        say()
        say("kernels alone on one batch (median of %d launches each, HIP events, the launches alternate)" % args.reps)
        ds.get(size)
        _images, _labels, index = ds.buffers(size)
        params, keys = ds._params[size], ds._keys[size]
        truth, ntruth = ds._lists[size]
        ptr = lambda t: C.c_void_p(t.data_ptr())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        head = (ptr(ds.boxes), ptr(ds.counts), ptr(ds.table), ptr(index), ptr(params))
        tail = (B, ds.max_obj, size, T, ptr(truth), ptr(ntruth), stream)
        calls = {"encode_box_list": lambda: _lib.check(lib.y2_encode_box_list(*head, *tail)),
                 "draw, keys": lambda: _lib.check(lib.y2_encode_box_list_draw(*head, ptr(keys), *tail)),
                 "draw, keys = NULL": lambda: _lib.check(lib.y2_encode_box_list_draw(*head, None, *tail))}
        ktimes = {k: [] for k in calls}
        for fn in calls.values():
            event_us(fn, args.warmup, 0)
        for _ in range(args.reps):
            for k, fn in calls.items():
                ktimes[k] += event_us(fn, 0, 1)
        cut = int((ntruth.cpu().numpy() == T).sum())
        say("%d of the batch's %d slots hold max_boxes rows" % (cut, B))
        for k, v in ktimes.items():
            say("%-18s %7.1f us" % (k, statistics.median(v)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
