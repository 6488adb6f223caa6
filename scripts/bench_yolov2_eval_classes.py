"""What per-class detection rows cost in a YOLOv2 evaluation batch (csrc/detect.hip: y2_detect_anchor_classes_batch),
batch 32 at 416 x 416 (845 candidates per image) and 608 x 608 (1805); the sibling of bench_yolov2_eval.py:

  (p) classes   y2_detect_anchor_classes_batch: one workgroup per (class, image), compacted sort, one launch
  (q) match     y2_voc_match_batch over the n * C segments of (p)'s rows, the index vector made on the device
  (a) anchor    y2_detect_anchor_batch on the same head tensor (one row per candidate: one workgroup per image)
  (c) forward   YOLOv2Detector.forward on a uint8 batch (moving statistics), full width

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  Two head tensors: `dense` (bench_yolov2_eval.py's random heads: most (candidate, class) scores
pass the 0.005 threshold) and `sparse` (objectness around sigmoid(-6) except --objects anchors per image that are sure
of one class: what 0.005 leaves of a trained head).  The claims under test: (p) + (q) stays below (c); the ratio (p) / (a)
and sparse against dense are recorded.

    python scripts/bench_yolov2_eval_classes.py --out profiles/yolov2_eval_classes.txt
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

    n, B, C, max_out, M = args.batch, 5, 20, 100, args.max_per_class
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    shapes = [(375, 500), (500, 375), (333, 500), (500, 334)]
    table = torch.from_numpy(np.array([(0,) + shapes[k % 4] + (1504, 0) for k in range(n)], np.int64)).cuda()
    index = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    seg_index = torch.empty(n * C, dtype=torch.int32, device="cuda")
    max_obj = 8
    boxes = np.zeros((n, max_obj, 5))
    for k in range(n):
        x, y = rng.integers(1, 200, (2, max_obj))
        boxes[k] = np.stack([x, y, x + rng.integers(20, 150, max_obj), y + rng.integers(20, 150, max_obj),
                             rng.integers(0, C, max_obj)], axis=1)
    gt = (torch.from_numpy(boxes).cuda(), torch.full((n,), max_obj, dtype=torch.int32, device="cuda"),
          torch.zeros((n, max_obj), dtype=torch.uint8, device="cuda"))
    say("YOLOv2 evaluation with per-class rows, batch %d, %s forward, score > 0.005, NMS 0.45, max_per_class %d (anchor "
        "rows: max_out %d); HIP events, median of %d alternating blocks of %d calls, milliseconds per call"
        % (n, args.dtype, M, max_out, args.reps, args.inner))
    say("size  head    candidates  valid/seg  rows/img  saturated  (p) classes  (q) match  (p)+(q)  (a) anchor  "
        "(c) forward  (p)/(a)")
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        K = S * S * B
        detector = None if args.no_forward else yolov2.YOLOv2Detector(n, size, dtype=args.dtype)
        images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
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
            out = E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M)
            flags = torch.empty((n * C, M), dtype=torch.int32, device="cuda")
            anchor_out = E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out)
            scores = E.decode_anchors(net, yolov2.ANCHORS_VOC)[1]
            valid_per_seg = float((scores > 0.005).float().sum()) / (n * C)      # (before the box checks)

            def classes():
                E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, out=out)

            def match():
                seg_index.view(n, C).copy_(index[:, None].expand(n, C))
                E.voc_match_batch(out[0].view(n * C, M, 6), out[1].view(n * C, M), out[2].view(-1), gt[0], gt[1], gt[2],
                                  seg_index, 0.5, out=flags)

            def anchor():
                E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out, out=anchor_out)

            def forward():
                detector.forward(images)

            legs = [("p", classes), ("q", match), ("a", anchor)] + ([] if detector is None else [("c", forward)])
            for _name, fn in legs:                               # warm-up: kernel loads, LDS attributes, filter packs
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _fn in legs}
            for _ in range(args.reps):
                for name, fn in legs:
                    ms[name].append(block_ms(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            count = out[2].cpu().numpy()
            say("%4d  %-6s  %10d  %9.1f  %8.1f  %4d/%4d  %11.4f  %9.4f  %7.4f  %10.4f  %11s  %7.2f" % (
                size, kind, K, valid_per_seg, count.sum() / n, int((count >= M).sum()), n * C, med["p"], med["q"],
                med["p"] + med["q"], med["a"], "%.4f" % med["c"] if "c" in med else "-", med["p"] / med["a"]))
        del detector
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
