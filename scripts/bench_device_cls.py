"""What the device-resident classifier batches cost (img_dataset/device_cls.py, y2_warp_u8_batch of csrc/augment.hip), on a
seeded list of synthetic 500 x 375 / 375 x 500 images, at batch 128 / 224 x 224 and batch 64 / 448 x 448:

  kernels   microseconds of y2_warp_u8_batch with rows drawn at the default ClsAugment next to y2_augment_u8_batch with
            rows drawn at the default Augment, on the SAME entries and output size, and y2_warp_u8_batch without
            parameters next to y2_resize_bilinear_u8_batch; HIP events around each launch, the launches alternate inside
            every repetition, median.  The ratio is recorded, not gated.
  paths     the share of (slot, tile) pairs of drawn batches that read the pool in place, are staged in LDS, or are fill
            alone (augment_cls.tile_path, the restatement of the kernel's rule)
  step      the f16 ClassifierTrainer.step fed from get(size) against the same step on one resident uint8 batch: blocks
            of steps alternate between the two, HIP events around every step, median over all blocks; and the host time of
            draw_batch alone

    python scripts/bench_device_cls.py --out profiles/device_cls.txt
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

from bench_device_voc import event_us  # noqa: E402


def make_list(root, count, seed):
    """`count` PNG files of seeded smooth-plus-noise pixels, alternately 500 x 375 and 375 x 500 -> [(path, label)]"""
    from PIL import Image
    rng = np.random.default_rng(seed)
    items = []
    for k in range(count):
        h, w = ((375, 500), (500, 375))[k % 2]
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(xx * (1 + k % 3) + yy) % 256, (yy * 2 + k) % 256, (xx + yy * (1 + k % 5)) % 256], axis=-1)
        img = ((base + rng.integers(0, 32, (h, w, 3))) % 256).astype(np.uint8)
        path = os.path.join(root, "im%04d.png" % k)
        Image.fromarray(img).save(path, compress_level=1)
        items.append((path, int(rng.integers(0, 1000))))
    return items


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--settings", default="128x224,64x448", help="batch x size, comma separated")
    ap.add_argument("--reps", type=int, default=30, help="timed launches per kernel (median)")
    ap.add_argument("--path-batches", type=int, default=4, help="drawn batches whose tiles are classified")
    ap.add_argument("--blocks", type=int, default=3, help="alternating blocks per variant")
    ap.add_argument("--steps", type=int, default=10, help="timed steps per block")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import _lib, trainer
    from tensorflow_yolo2_amd.img_dataset import augment_cls as AC
    from tensorflow_yolo2_amd.img_dataset.augment import Augment, generator
    from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    lib = _lib.load()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with tempfile.TemporaryDirectory() as tmp:
        items = make_list(tmp, args.images, seed=0)
        for setting in args.settings.split(","):
            batch, size = (int(v) for v in setting.split("x"))
            t0 = time.perf_counter()
            aug = AC.ClsAugment()
            ds = DeviceCls(items, batch, seed=0, augment=aug)
            torch.cuda.synchronize()
            say("device_cls, batch %d at %d x %d, %d images, pool %.1f MB, start-up %.2f s; %r"
                % (batch, size, size, len(ds.entries), ds.pool_bytes / 1e6, time.perf_counter() - t0, aug))
            table = ds.table.cpu().numpy()
            images, labels, index, params = ds.buffers(size)
            entries = np.array([ds._next()['entry'] for _ in range(batch)], np.int32)
            rows = aug.draw_batch(ds.aug_rng, ds.shapes[entries], size)
            old = Augment()
            old_rng = generator(0, 0)
            old_rows = torch.from_numpy(np.array([old.draw(old_rng, table[e, 1], table[e, 2]) for e in entries])).cuda()
            index.copy_(torch.from_numpy(entries))
            params.copy_(torch.from_numpy(rows))
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            calls = {
                "resize": lambda: _lib.check(lib.y2_resize_bilinear_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), batch, size, size, ptr(images), stream)),
                "warp_plain": lambda: _lib.check(lib.y2_warp_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), None, ptr(ds.labels), batch, size, size, 127, ptr(images),
                    ptr(labels), stream)),
                "augment": lambda: _lib.check(lib.y2_augment_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), ptr(old_rows), batch, size, size, old.fill, ptr(images),
                    stream)),
                "warp": lambda: _lib.check(lib.y2_warp_u8_batch(
                    ptr(ds.pool), ptr(ds.table), ptr(index), ptr(params), ptr(ds.labels), batch, size, size, aug.fill,
                    ptr(images), ptr(labels), stream)),
            }
            times = {k: [] for k in calls}
            for fn in calls.values():
                event_us(fn, args.warmup, 0)
            for _ in range(args.reps):
                for k, fn in calls.items():
                    times[k] += event_us(fn, 0, 1)
            t = {k: statistics.median(v) for k, v in times.items()}
            say("kernels (median of %d launches each, HIP events, the four launches alternate)" % args.reps)
            say("resize_us  warp_plain_us  warp_plain/resize  augment_us  warp_us  warp/augment  batch_MB  warp_GB/s_written")
            say("%9.1f  %13.1f  %17.2f  %10.1f  %7.1f  %12.2f  %8.1f  %17.1f"
                % (t["resize"], t["warp_plain"], t["warp_plain"] / t["resize"], t["augment"], t["warp"],
                   t["warp"] / t["augment"], images.numel() / 1e6, images.numel() / (t["warp"] * 1e-6) / 1e9))
            count = {"inplace": 0, "staged": 0, "fill": 0}
            tiles = (size + AC.TILE - 1) // AC.TILE
            rng = AC.generator(1, 0)
            for _ in range(args.path_batches):
                es = np.array([ds._next()['entry'] for _ in range(batch)], np.int32)
                for e, r in zip(es, aug.draw_batch(rng, ds.shapes[es], size)):
                    off, h, w, pitch, _ = (int(x) for x in table[e])
                    for ty in range(tiles):
                        for tx in range(tiles):
                            count[AC.tile_path(h, w, pitch, off, r, size, size, tx, ty)] += 1
            total = float(sum(count.values()))
            say("paths over %d drawn batches (%d tiles): staged %.4f, in place %.4f, fill %.4f"
                % (args.path_batches, int(total), count["staged"] / total, count["inplace"] / total,
                   count["fill"] / total))
            t0 = time.perf_counter()
            for _ in range(50):
                aug.draw_batch(ds.aug_rng, ds.shapes[entries], size)
            say("host: draw_batch of %d rows alone: %.3f ms (wall clock, mean of 50 batches)"
                % (batch, (time.perf_counter() - t0) / 50 * 1e3))
            if not args.skip_steps:
                tr = trainer.ClassifierTrainer(batch, size, dtype="f16")
                resident_i, resident_l = (x.clone() for x in ds.get(size))
                fed_resident = lambda: tr.step(resident_i, resident_l)
                fed_pool = lambda: tr.step(*ds.get(size))
                times = {"resident": [], "pool": []}
                for fn in (fed_resident, fed_pool):
                    event_us(fn, args.warmup, 0)
                for _ in range(args.blocks):
                    times["resident"] += event_us(fed_resident, 1, args.steps)
                    times["pool"] += event_us(fed_pool, 1, args.steps)
                p, a = statistics.median(times["resident"]) / 1e3, statistics.median(times["pool"]) / 1e3
                say("f16 ClassifierTrainer.step (median of %d x %d steps per variant, alternating blocks, HIP events)"
                    % (args.blocks, args.steps))
                say("resident_ms  from_get_ms  difference_us  from_get/resident")
                say("%11.3f  %11.3f  %13.1f  %17.4f" % (p, a, (a - p) * 1e3, a / p))
                del tr, fed_resident, fed_pool
            say()
            del ds
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
