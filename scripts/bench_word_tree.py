"""What the word tree of the region layer costs at the training shape: batch 64, heads of 416 x 416 (S = 13) and 608 x 608
(S = 19), 5 anchors, 400 classes (a head of 2,025 columns), a generated tree of depth 6:

  (f) flat loss   y2_yolov2_loss_boxes at the same N, S, B and C: the parent commit's kernel, the baseline -- one thread
                  walks and writes a whole (cell, anchor) row of 405 floats
  (t) tree loss   y2_yolov2_loss_boxes_tree on the same head and box lists: rows written with consecutive lanes on
                  consecutive floats, a wave per owned row on the truth's path
  (h) head        y2_word_tree_head over all N S S B rows, out of place
  (d) detect      engine.word_tree_head (in place) + engine.detect_anchor_classes_batch on that head: one row per
                  (candidate, class), 400 workgroups per image

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  Bytes: a loss reads `net` once at most and writes `dnet` once, 2 N S S B (5 + C) 4; the head
reads and writes the same.  The claim under test: (t) is no slower than (f).

    python scripts/bench_word_tree.py --out profiles/word_tree.txt
"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_TBS = 5.0                    # what the streaming kernels of this library reach


def generated_tree(n, depth, seed=0):
    """a tree of n nodes and the given largest depth: 8 roots, then an equal share of the nodes per level, in runs of
    random width (1..24) under random nodes of the level above"""
    import numpy as np
    from tensorflow_yolo2_amd.utils import word_tree
    rng = np.random.default_rng(seed)
    parent = [-1] * 8
    level = list(range(8))
    per_level = (n - 8) // depth
    for d in range(1, depth + 1):
        want = per_level if d < depth else n - len(parent)
        new = []
        order = rng.permutation(level)
        for at, p in enumerate(order):
            if want <= 0:
                break
            k = want if at == len(order) - 1 else int(min(want, rng.integers(1, 25)))   # (the last parent takes the rest)
            new += list(range(len(parent), len(parent) + k))
            parent += [int(p)] * k
            want -= k
        level = new
    tree = word_tree.parse("".join("n%d %d\n" % (i, p) for i, p in enumerate(parent)), "<generated>")
    assert tree.n == n and tree.max_depth == depth, (tree.n, tree.max_depth)
    return tree


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--sizes", default="416,608")
    ap.add_argument("--classes", type=int, default=400)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--detect-inner", type=int, default=2)
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
            fn()
        torch.cuda.synchronize()
        us = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                us[name].append(block_us(fn, inner))
        return {k: statistics.median(v) for k, v in us.items()}

    n, B, Cn, T = args.batch, 5, args.classes, 30
    tree = generated_tree(Cn, args.depth)
    tt = E.WordTreeTables(tree)
    ptr, stream = E._ptr, E._stream
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    say("Word tree, batch %d, %d anchors, %d classes in %d groups (largest %d), depth %d; HIP events, median of %d "
        "alternating blocks, microseconds per call (a loss: kernel + finalize); bytes against %.1f TB/s"
        % (n, B, Cn, tt.groups, int(tree.group_size.max()), tree.max_depth, args.reps, STREAM_TBS))
    say("size  rows  truths/img  MB (read + write)  us at %.0f TB/s  (f) flat loss  (t) tree loss  (t)/(f)  (h) head  "
        "(d) head + per-class detect" % STREAM_TBS)
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        rows = n * S * S * B
        net = torch.from_numpy((rng.standard_normal((n, S, S, B, 5 + Cn)) * 0.7).astype(np.float32)).cuda()
        full = np.zeros((n, T, 5), np.float32)
        full[..., 0:2] = rng.uniform(1, size - 1, (n, T, 2))
        full[..., 2:4] = rng.uniform(0.05 * size, 0.6 * size, (n, T, 2))
        full[..., 4] = rng.integers(0, Cn, (n, T))
        count = rng.integers(1, 13, n).astype(np.int32)              # 1..12 objects per image
        truth, ntruth = torch.from_numpy(full).cuda(), torch.from_numpy(count).cuda()
        loss, dnet, out = torch.empty(5, device="cuda"), torch.empty_like(net), torch.empty_like(net)
        ws = torch.empty(lib.y2_yolov2_loss_boxes_tree_workspace_bytes(n, S, B) + 4096, dtype=torch.uint8, device="cuda")
        sc = (C.c_float * 7)(1.0, 5.0, 1.0, 1.0, 0.6, 1.0, 0.01)
        table = torch.from_numpy(np.array([(0, 375, 500, 1504, 0)] * n, np.int64)).cuda()
        det = (torch.empty((n, Cn, 8, 6), dtype=torch.int32, device="cuda"),
               torch.empty((n, Cn, 8), dtype=torch.float32, device="cuda"),
               torch.empty((n, Cn), dtype=torch.int32, device="cuda"))

        def flat_loss():
            E.check(lib.y2_yolov2_loss_boxes(ptr(net), ptr(truth), ptr(ntruth), ptr(anchors), n, S, B, Cn, T, float(size),
                                             sc, ptr(loss), ptr(dnet), ptr(ws), stream()))

        def tree_loss():
            E.check(lib.y2_yolov2_loss_boxes_tree(ptr(net), ptr(truth), ptr(ntruth), ptr(anchors), ptr(tt.tables), n, S, B,
                                                  Cn, tt.groups, tt.max_depth, T, float(size), sc, ptr(loss), ptr(dnet),
                                                  ptr(ws), stream()))

        def head():
            E.check(lib.y2_word_tree_head(ptr(net), ptr(tt.tables), rows, Cn, tt.groups, tt.max_depth, 0.5, ptr(out), None,
                                          None, stream()))

        def detect():
            E.word_tree_head(net, tt, 0.5, out=out)
            E.detect_anchor_classes_batch(out, anchors, table, None, 0.005, 0.45, 8, out=det)

        med = medians([("f", flat_loss), ("t", tree_loss), ("h", head)], args.inner)
        med.update(medians([("d", detect)], args.detect_inner))
        mb = 2 * rows * (5 + Cn) * 4 / 1e6
        say("%4d  %6d  %10.1f  %17.1f  %14.1f  %13.1f  %13.1f  %7.2f  %8.1f  %27.1f"
            % (size, rows, float(count.mean()), mb, mb / STREAM_TBS, med["f"], med["t"], med["t"] / med["f"], med["h"],
               med["d"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
