"""What the post-processing of a YOLOv2 evaluation batch costs (csrc/detect.hip: y2_detect_anchor_batch), batch 32 at
416 x 416 (845 candidates per image) and 608 x 608 (1805: two slots per lane):

  (a) fused     y2_detect_anchor_batch: decode, class choice, pixels of the original image, class-aware NMS, one launch
  (b) three     y2_decode_anchors + y2_class_argmax + y2_nms (class-aware) on the same head tensor: the launches (a)
                replaces.  (b) stops at keep-indices into relative boxes and is NOT the same function; it is the work
                the detect() path does for the same candidates
  (m) match     y2_voc_match_batch on (a)'s rows
  (c) forward   YOLOv2Detector.forward on a uint8 batch (moving statistics), full width

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  Two head tensors: `dense` (random heads: almost every candidate passes the 0.005 threshold, the
longest NMS walk) and `sparse` (objectness around sigmoid(-6): a few candidates per image, as a trained net gives).  The
claims under test: (a) is no slower than (b); (a) + (m) stays below (c).

    python scripts/bench_yolov2_eval.py --out profiles/yolov2_eval.txt [--append FILE ...]
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
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--append", nargs="*", default=[], help="text files whose lines are copied under the table")
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

    n, B, C, max_out = args.batch, 5, 20, 100
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    shapes = [(375, 500), (500, 375), (333, 500), (500, 334)]
    table = torch.from_numpy(np.array([(0,) + shapes[k % 4] + (1504, 0) for k in range(n)], np.int64)).cuda()
    index = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    max_obj = 8
    boxes = np.zeros((n, max_obj, 5))
    for k in range(n):
        x, y = rng.integers(1, 200, (2, max_obj))
        boxes[k] = np.stack([x, y, x + rng.integers(20, 150, max_obj), y + rng.integers(20, 150, max_obj),
                             rng.integers(0, C, max_obj)], axis=1)
    gt = (torch.from_numpy(boxes).cuda(), torch.full((n,), max_obj, dtype=torch.int32, device="cuda"),
          torch.zeros((n, max_obj), dtype=torch.uint8, device="cuda"))
    say("YOLOv2 evaluation post-processing, batch %d, %s forward, score > 0.005, NMS 0.45, max_out %d; HIP events, "
        "median of %d alternating blocks of %d calls, milliseconds per call" % (n, args.dtype, max_out, args.reps, args.inner))
    say("size  head    candidates  kept/img  (a) fused  (b) three launches  (m) match  (a)+(m)  (c) forward  (b)/(a)")
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        detector = None if args.no_forward else yolov2.YOLOv2Detector(n, size, dtype=args.dtype)
        images = torch.from_numpy(rng.integers(0, 256, (n, size, size, 3), dtype=np.uint8)).cuda()
        for kind in ("dense", "sparse"):
            head = rng.normal(0.0, 1.0, (n, S, S, B, 5 + C)).astype(np.float32)
            head[..., 2:4] = rng.uniform(-1.5, 0.5, (n, S, S, B, 2))
            head[..., 5:] *= 2.0
            if kind == "sparse":
                head[..., 4] = rng.normal(-6.0, 1.5, (n, S, S, B))
            net = torch.from_numpy(head).cuda()
            out = E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out)
            flags = torch.empty((n, max_out), dtype=torch.int32, device="cuda")
            K = S * S * B
            bx = torch.empty((n, K, 4), dtype=torch.float32, device="cuda")
            sc = torch.empty((n, K, C), dtype=torch.float32, device="cuda")
            best = torch.empty((n, K), dtype=torch.float32, device="cuda")
            cls = torch.empty((n, K), dtype=torch.int32, device="cuda")
            keep = torch.empty((n, max_out), dtype=torch.int32, device="cuda")
            cnt = torch.empty((n,), dtype=torch.int32, device="cuda")
            lib, ptr, stream = E._lib.load(), E._ptr, E._stream

            def fused():
                E.detect_anchor_batch(net, anchors, table, index, 0.005, 0.45, max_out, out=out)

            def three():                                         # the C ABI on tensors allocated once, as (a) is
                E.check(lib.y2_decode_anchors(ptr(net), ptr(anchors), ptr(bx), ptr(sc), n, S, B, C, stream()))
                E.check(lib.y2_class_argmax(ptr(sc), ptr(best), ptr(cls), n * K, C, stream()))
                E.check(lib.y2_nms(ptr(bx), ptr(best), ptr(cls), n, K, 0.45, 0.005, max_out, 1, ptr(keep), ptr(cnt), stream()))

            def match():
                E.voc_match_batch(out[0], out[1], out[2], gt[0], gt[1], gt[2], index, 0.5, out=flags)

            def forward():
                detector.forward(images)

            legs = [("a", fused), ("b", three), ("m", match)] + ([] if detector is None else [("c", forward)])
            for _name, fn in legs:                               # warm-up: kernel loads, LDS attributes, filter packs
                fn()
            torch.cuda.synchronize()
            ms = {name: [] for name, _fn in legs}
            for _ in range(args.reps):
                for name, fn in legs:
                    ms[name].append(block_ms(fn))
            med = {k: statistics.median(v) for k, v in ms.items()}
            kept = float(out[2].float().mean())
            say("%4d  %-6s  %10d  %8.1f  %9.4f  %18.4f  %9.4f  %7.4f  %11s  %7.2f" % (
                size, kind, S * S * B, kept, med["a"], med["b"], med["m"], med["a"] + med["m"],
                "%.4f" % med["c"] if "c" in med else "-", med["b"] / med["a"]))
        del detector
    for path in args.append:
        if os.path.isfile(path):
            say()
            with open(path) as f:
                for line in f.read().splitlines():
                    say(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
