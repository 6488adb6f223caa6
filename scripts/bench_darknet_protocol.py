"""What Darknet's test-time protocol costs in a YOLOv2 evaluation batch (csrc/darknet_io.hip), batch 32 at 416 x 416 and
608 x 608; the sibling of bench_letterbox.py:

  (l) + (u)     y2_letterbox_u8_batch then y2_u8_bgr_to_f32_rgb: the pair that makes the network's float input today
  (d)           y2_letterbox_darknet_batch on the same entries: one launch from the pool to the float input
  (P) / (D)     y2_detect_anchor_classes_batch_lb / y2_detect_anchor_classes_batch_dk on the same head tensor
  (q) / (Q)     y2_voc_match_batch over (P)'s rows / y2_voc_match_batch_f over (D)'s rows

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.  The pool holds --batch images of VOC's usual shapes (random bytes); the head tensors are
bench_letterbox.py's `dense` and `sparse`.  The claims under test: (d) is no slower than (l) + (u); (D) is within the
box-to-box spread (4 %) of (P), and (Q) of (q).

    python scripts/bench_darknet_protocol.py --out profiles/darknet_protocol.txt
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--max-per-class", type=int, default=32)
    ap.add_argument("--objects", type=int, default=40, help="confident anchors per image of the sparse head")
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
        for _name, fn in legs:                                   # warm-up: kernel loads, LDS attributes
            fn()
        torch.cuda.synchronize()
        ms = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                ms[name].append(block_ms(fn))
        return {k: statistics.median(v) for k, v in ms.items()}

    n, B, C, M = args.batch, 5, 20, args.max_per_class
    anchors = torch.as_tensor(np.asarray(yolov2.ANCHORS_VOC, np.float32)).cuda()
    rng = np.random.default_rng(0)
    shapes = [((375, 500), (500, 375), (333, 500), (500, 334))[k % 4] for k in range(n)]
    offsets, pitches, total = pool_layout(shapes)
    pool = torch.from_numpy(rng.integers(0, 256, total, dtype=np.uint8)).cuda()
    table = torch.from_numpy(np.array([(off, h, w, pitch, 0) for (h, w), off, pitch in zip(shapes, offsets, pitches)],
                                      np.int64)).cuda()
    index = torch.from_numpy(rng.permutation(n).astype(np.int32)).cuda()
    seg_index = index[:, None].expand(n, C).contiguous().view(-1)
    max_obj = 8
    boxes = np.zeros((n, max_obj, 5))
    for k in range(n):
        x, y = rng.integers(1, 200, (2, max_obj))
        boxes[k] = np.stack([x, y, x + rng.integers(20, 150, max_obj), y + rng.integers(20, 150, max_obj),
                             rng.integers(0, C, max_obj)], axis=1)
    gt = (torch.from_numpy(boxes).cuda(), torch.full((n,), max_obj, dtype=torch.int32, device="cuda"),
          torch.zeros((n, max_obj), dtype=torch.uint8, device="cuda"))
    say("YOLOv2 under Darknet's test-time protocol, batch %d, score > 0.005, NMS 0.45, max_per_class %d; HIP events, "
        "median of %d alternating blocks of %d calls, milliseconds per call" % (n, M, args.reps, args.inner))
    for size in [int(v) for v in args.sizes.split(",")]:
        S = size // 32
        K = S * S * B
        images = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        floats = torch.empty((n, size, size, 3), dtype=torch.float32, device="cuda")
        floats_d = torch.empty((n, size, size, 3), dtype=torch.float32, device="cuda")

        def pair():
            E.letterbox_batch(pool, table, index, n, size, 127, out=images)
            E.u8_to_darknet_input(images, out=floats)

        med = medians([("l", lambda: E.letterbox_batch(pool, table, index, n, size, 127, out=images)),
                       ("u", lambda: E.u8_to_darknet_input(images, out=floats)),
                       ("lu", pair),
                       ("d", lambda: E.letterbox_darknet_batch(pool, table, index, n, size, out=floats_d))])
        say("size %4d  images  (l) letterbox_u8 %.4f  (u) u8_to_f32 %.4f  (l)+(u) in one block %.4f  (d) letterbox_darknet "
            "%.4f  (d)/((l)+(u)) %.3f" % (size, med["l"], med["u"], med["lu"], med["d"], med["d"] / med["lu"]))
        say("size  head    candidates  (P) classes_lb  (D) classes_dk  (D)/(P)  (q) match  (Q) match_f  (Q)/(q)")
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
            P_out = E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, net_size=size)
            D_out = E.detect_anchor_classes_batch_darknet(net, anchors, table, index, 0.005, 0.45, M, net_size=size)
            flags = torch.empty((n * C, M), dtype=torch.int32, device="cuda")
            flags_f = torch.empty((n * C, M), dtype=torch.int32, device="cuda")
            views = lambda out: (out[0].view(n * C, M, 6), out[1].view(n * C, M), out[2].view(-1))
            legs = [
                ("P", lambda: E.detect_anchor_classes_batch(net, anchors, table, index, 0.005, 0.45, M, out=P_out,
                                                            net_size=size)),
                ("D", lambda: E.detect_anchor_classes_batch_darknet(net, anchors, table, index, 0.005, 0.45, M,
                                                                    out=D_out, net_size=size)),
                ("q", lambda: E.voc_match_batch(*views(P_out), gt[0], gt[1], gt[2], seg_index, 0.5, out=flags)),
                ("Q", lambda: E.voc_match_batch_f(*views(D_out), gt[0], gt[1], gt[2], seg_index, 0.5, out=flags_f))]
            med = medians(legs)
            say("%4d  %-6s  %10d  %14.4f  %14.4f  %7.3f  %9.4f  %11.4f  %7.3f" % (
                size, kind, K, med["P"], med["D"], med["D"] / med["P"], med["q"], med["Q"], med["Q"] / med["q"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
