"""What letterboxed inference costs in a YOLOv2 evaluation batch (csrc/data.hip: y2_letterbox_u8_batch; csrc/detect.hip:
y2_detect_anchor_batch_lb, y2_detect_anchor_classes_batch_lb), batch 32 at 416 x 416 and 608 x 608; the sibling of
bench_yolov2_eval_classes.py:

  (r) resize    y2_resize_bilinear_u8_batch: the plain stretch of the same pool entries
  (l) letterbox y2_letterbox_u8_batch on the same entries
  (a) / (A)     y2_detect_anchor_batch / y2_detect_anchor_batch_lb on the same head tensor
  (p) / (P)     y2_detect_anchor_classes_batch / y2_detect_anchor_classes_batch_lb on the same head tensor
  (q) match     y2_voc_match_batch over (A)'s rows
  (c) forward   YOLOv2Detector.forward on the letterboxed uint8 batch (moving statistics), full width

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  The pool holds --batch images of VOC's usual shapes (random bytes); the head tensors are
bench_yolov2_eval_classes.py's `dense` and `sparse`.  The claims under test: (l) is no slower than (r); (A) and (P) are
within the box-to-box spread (4 %) of (a) and (p); (l) + (A) + (q) stays below (c).

    python scripts/bench_letterbox.py --out profiles/letterbox.txt
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
    ap.add_argument("--max-per-class", type=int, default=32)
    ap.add_argument("--objects", type=int, default=40, help="confident anchors per image of the sparse head")
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.img_dataset.device_voc import pool_layout
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def block_ms(fn):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / args.inner

    def medians(legs):
        for _name, fn in legs:                                   # warm-up: kernel loads, LDS attributes, filter packs
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                ms[name].append(block_ms(fn))
        return {k: statistics.median(v) for k, v in ms.items()}

    n, B, C, max_out, M = args.batch, 5, 20, 100, args.max_per_class
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    shapes = [((375, 500), (500, 375), (333, 500), (500, 334))[k % 4] for k in range(n)]
    offsets, pitches, total = pool_layout(shapes)
    pool = torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)).cuda()
    table = torch.from_numpy(np.array([(off, h, w, pitch, 0) for (h, w), off, pitch in zip(shapes, offsets, pitches)],
                                      np.int64)).cuda()
    index = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    max_obj = 8
    boxes = np.zeros((n, max_obj, 5))
    for k in range(n):
        x, y = rng.integers(1, 200, (2, max_obj))
        boxes[k] = np.stack([x, y, x + rng.integers(20, 150, max_obj), y + rng.integers(20, 150, max_obj),
                             rng.integers(0, C, max_obj)], axis=1)
    gt = (torch.from_numpy(boxes).cuda(), torch.full((n,), max_obj, dtype=torch.int32, device="cuda"),
          torch.zeros((n, max_obj), dtype=torch.uint8, device="cuda"))
    say("YOLOv2 letterboxed inference, batch %d, %s forward, score > 0.005, NMS 0.45, max_out %d, max_per_class %d; HIP "
        "events, median of %d alternating blocks of %d calls, milliseconds per call"
        % (n, args.dtype, max_out, M, args.reps, args.inner))
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        K = S * S * B
        images = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        lib = E._lib.load()

        def resize():
            E.check(lib.y2_resize_bilinear_u8_batch(E._ptr(pool), E._ptr(table), E._ptr(index), n, size, size,
                                                    E._ptr(images), E._stream()))

        def letterbox():
            E.letterbox_batch(pool, table, index, n, size, 127, out=images)

        med = medians([("r", resize), ("l", letterbox)])
        say("size %4d  images  (r) resize %.4f  (l) letterbox %.4f  (l)/(r) %.3f" % (size, med["r"], med["l"],
                                                                                    med["l"] / med["r"]))
        l_ms = med["l"]
        c_ms = None
        if not args.no_forward:
            detector = yolov2.YOLOv2Detector(n, size, dtype=args.dtype)
            letterbox()
            c_ms = medians([("c", lambda: detector.forward(images))])["c"]
            del detector
        say("size  head    candidates  (a) anchor  (A) anchor_lb  (A)/(a)  (p) classes  (P) classes_lb  (P)/(p)  "
            "(q) match  (l)+(A)+(q)  (c) forward")
        for kind in ("dense", "sparse"):
            head = rng.normal(0.0, 1.0, (n, S, S, B, 5 + C)).astype(np.float32)
            head[..., 2:4] = rng.uniform(-1.5, 0.5, (n, S, S, B, 2))
            head[..., 5:] *= 2.0
            if kind == "sparse":
                flat = head.reshape(n, K, 5 + C)
                flat[..., 4] = rng.normal(-6.0, 0.5, (n, K))
                for k in range(n):
                    sure = rng.choice(K, args.objects, replace=False)
                    flat[k, sure, 4] = rng.normal(2.0, 1.0, args.objects)
                    flat[k, sure, 5 + rng.integers(0, C, args.objects)] += 6.0
            net = torch.from_numpy(head).cuda()
            a_out = E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out)
            A_out = E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out, net_size=size)
            p_out = E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M)
            P_out = E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, net_size=size)
            flags = torch.empty((n, max_out), dtype=torch.int32, device="cuda")
            legs = [
                ("a", lambda: E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out, out=a_out)),
                ("A", lambda: E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out, out=A_out,
                                                    net_size=size)),
                ("p", lambda: E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, out=p_out)),
                ("P", lambda: E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, out=P_out,
                                                            net_size=size)),
                ("q", lambda: E.voc_match_batch(A_out[0], A_out[1], A_out[2], gt[0], gt[1], gt[2], index, 0.5,
                                                out=flags))]
            med = medians(legs)
            say("%4d  %-6s  %10d  %10.4f  %13.4f  %7.3f  %11.4f  %14.4f  %7.3f  %9.4f  %11.4f  %11s" % (
                size, kind, K, med["a"], med["A"], med["A"] / med["a"], med["p"], med["P"], med["P"] / med["p"],
                med["q"], l_ms + med["A"] + med["q"], "%.4f" % c_ms if c_ms is not None else "-"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
