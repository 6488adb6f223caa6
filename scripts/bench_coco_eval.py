"""What COCO's matching costs in a YOLOv2 evaluation batch (csrc/coco.hip), batch 32 at 416 x 416, 80 classes, 100 rows per
(image, class); the sibling of bench_darknet_protocol.py:

  (a) the launch   (D) y2_detect_anchor_classes_batch_dk on a head tensor, (M) y2_coco_match_batch over its rows -- ten
                   thresholds x four area ranges, forty walks -- and (Q) y2_voc_match_batch_f over the SAME rows: one
                   threshold, one walk.  The ground truth is one table of objects in both conventions.
  (b) the batch    y2_letterbox_darknet_batch -> YOLOv2Detector.forward of --cfg (yolov2.cfg, f16, initial weights) ->
                   (D) -> (M), with and without (M).  The detect launch reads the head tensor of (a), not the forward
                   pass's own output, so that the rows are the same in both parts; the forward pass is run and timed.

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  The head tensors are bench_letterbox.py's `dense` and `sparse` at 80 classes.  The claim under
test: the match is small beside the forward pass of its batch.

    python scripts/bench_coco_eval.py --out profiles/coco_eval.txt
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
    ap.add_argument("--size", type=int, default=416)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch-inner", type=int, default=3)
    ap.add_argument("--max-per-class", type=int, default=100)
    ap.add_argument("--objects", type=int, default=40, help="confident anchors per image of the sparse head")
    ap.add_argument("--max-obj", type=int, default=24, help="annotations per image: 1 .. this many (COCO's mean is 7)")
    ap.add_argument("--cfg", default=os.path.join(ROOT, "tests", "golden", "cfg", "yolov2.cfg"))
    ap.add_argument("--no-forward", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.img_dataset.device_voc import pool_layout
    from tensorflow_yolo2_amd.utils import coco_eval, darknet_cfg
    from tensorflow_yolo2_amd.yolo2_nets import yolov2
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    def block_ms(fn, inner):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / inner

    def medians(legs, inner):
        for _name, fn in legs:                                   # warm-up: kernel loads, LDS attributes
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                ms[name].append(block_ms(fn, inner))
        return {k: statistics.median(v) for k, v in ms.items()}

    rec = darknet_cfg.load(args.cfg)
    n, size, B, C, M = args.batch, args.size, rec.num, rec.classes, args.max_per_class
    S = size // 32
    K = S * S * B
    anchors = torch.as_tensor(np.asarray(rec.anchors, np.float32)).cuda()
    rng = np.random.default_rng(0)
    shapes = [((480, 640), (640, 480), (427, 640), (640, 426))[k % 4] for k in range(n)]
    offsets, pitches, total = pool_layout(shapes)
    pool = torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)).cuda()
    table = torch.from_numpy(np.array([(off, h, w, pitch, 0) for (h, w), off, pitch in zip(shapes, offsets, pitches)],
                                      np.int64)).cuda()
    index = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    seg_index = index[:, None].expand(n, C).contiguous().view(-1)
    # one set of objects, as COCO's x, y, w, h with area and crowd and as the devkit's 1-based inclusive corners
    max_obj = args.max_obj
    coco_boxes, voc_boxes = np.zeros((n, max_obj, 5)), np.zeros((n, max_obj, 5))
    for k in range(n):
        x, y = rng.integers(0, 300, (2, max_obj)).astype(np.float64)
        w, h = rng.integers(10, 300, (2, max_obj)).astype(np.float64)
        c = rng.integers(0, C, max_obj)
        coco_boxes[k] = np.stack([x, y, w, h, c], axis=1)
        voc_boxes[k] = np.stack([x + 1, y + 1, x + w, y + h, c], axis=1)
    counts = torch.from_numpy(rng.integers(1, max_obj + 1, n).astype(np.int32)).cuda()
    area = torch.from_numpy(coco_boxes[:, :, 2] * coco_boxes[:, :, 3] * rng.uniform(0.3, 1.0, (n, max_obj))).cuda()
    crowd = torch.from_numpy((rng.random((n, max_obj)) < 0.05).astype(np.uint8)).cuda()
    coco_gt = (torch.from_numpy(coco_boxes).cuda(), area, crowd, counts)
    voc_gt = (torch.from_numpy(voc_boxes).cuda(), counts, crowd)            # crowd stands in for `difficult`
    thresholds = torch.as_tensor(coco_eval.THRESHOLDS).cuda()
    ranges = torch.as_tensor(coco_eval.AREA_RANGES).cuda()
    A = ranges.shape[0]
    say("COCO matching in a YOLOv2 evaluation batch: batch %d at %d x %d, %d classes, score > 0.005, NMS 0.45, max_per_class "
        "%d, 1..%d annotations per image; HIP events, median of %d alternating blocks, milliseconds per call"
        % (n, size, size, C, M, max_obj, args.reps))
    detector = None
    if not args.no_forward:
        detector = yolov2.YOLOv2Detector.from_cfg(args.cfg, n, size, dtype="f16")
        floats = torch.empty((n, size, size, 3), dtype=torch.float32, device="cuda")
    say("(a) blocks of %d calls                                              (b) blocks of %d batches" % (args.inner, args.batch_inner))
    say("head    rows      (D) classes_dk  (M) coco_match  (Q) voc_match_f  (M)/(Q)  (M)/(D)   forward  batch  batch+(M)  "
        "(M) share of the batch")
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
        D_out = E.detect_anchor_classes_batch_darknet(net, anchors, table, index, 0.005, 0.45, M, net_size=size)
        det, score, count = D_out[0].view(n * C, M, 6), D_out[1].view(n * C, M), D_out[2].view(-1)
        match = torch.empty((n * C, M, A), dtype=torch.int32, device="cuda")
        flags = torch.empty((n * C, M), dtype=torch.int32, device="cuda")

        def detect():
            E.detect_anchor_classes_batch_darknet(net, anchors, table, index, 0.005, 0.45, M, out=D_out, net_size=size)

        def coco_match():
            E.coco_match_batch(det, count, *coco_gt, seg_index, thresholds, ranges, 1, out=match)

        med = medians([("D", detect), ("M", coco_match),
                       ("Q", lambda: E.voc_match_batch_f(det, score, count, *voc_gt, seg_index, 0.5, out=flags))], args.inner)
        text = "%-6s  %8d  %14.4f  %14.4f  %15.4f  %7.2f  %7.2f" % (
            kind, int(count.sum().item()), med["D"], med["M"], med["Q"], med["M"] / med["Q"], med["M"] / med["D"])
        if detector is not None:
            def batch():
                E.letterbox_darknet_batch(pool, table, index, n, size, out=floats)
                detector.forward(floats)
                detect()

            def batch_match():
                batch()
                coco_match()

            bm = medians([("f", lambda: detector.forward(floats)), ("b", batch), ("bm", batch_match)], args.batch_inner)
            text += "  %8.3f  %5.3f  %9.3f  %6.2f %% (from (a): %.2f %% of the forward pass)" % (
                bm["f"], bm["b"], bm["bm"], 100.0 * (bm["bm"] - bm["b"]) / bm["bm"], 100.0 * med["M"] / bm["f"])
        say(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
