"""What detection on YOLO9000's head costs from the class row and from the tree's node: K = 1024 -> 28,269 (3 anchors x
(5 + 9,418 nodes)), the generated 9,418-node tree, S = 17 (one 544 x 544 image: 867 candidates) at batch 1 and 32.  The
head is engine.WideHead's output on random operands, once as it comes ("random": objectness around 0.5, every candidate
passes 0.005) and once with the objectness bias at -8 ("trained": about 5 % of the candidates pass).

  (c)   engine.word_tree_head            the rewrite: every row to 0 at top, -inf elsewhere, into a second buffer
  (d)   engine.detect_anchor_batch       on those rows: a 9,418-wide softmax per candidate, twice
  (c')  engine.word_tree_top             the same walk, nothing rewritten: obj_thresh -1 (every row) and 0.005
  (d')  engine.detect_anchor_tree_batch  on the raw head and (c')'s top at 0.005
  (f)   engine.detect_anchor_batch       at num_class = 1 on the same five box values: the same decode, sort and walk with
                                         a one-wide class row -- the floor of (d')

The requirement: (c') + (d') below (c) + (d) at both batches.  The expectation written down before measuring (DESIGN.md 9,
"Detection from the node"): (d') lands near (f); what the row stride of 9,423 floats costs (one cache line per candidate
instead of shared lines) is what the ratio (d') / (f) shows.  An expectation, not a gate.  The rows of (d') are compared
with (d)'s bit for bit in the same run.

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported (a leg whose single call takes longer than 25 ms runs in blocks of 2).

    python scripts/bench_detect_tree.py --out profiles/detect_tree.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--cout", type=int, default=28269)
    ap.add_argument("--cells", type=int, default=289)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--anchors", type=int, default=3)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from bench_word_tree import generated_tree
    from tensorflow_yolo2_amd import engine as E
    assert torch.cuda.is_available(), "needs the MI355X"
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

    def medians(legs):
        inner = {}
        for name, fn in legs:
            fn()
            torch.cuda.synchronize()
            inner[name] = args.inner if block_us(fn, 1) < 25e3 else 2
        us = {name: [] for name, _fn in legs}
        for _ in range(args.reps):
            for name, fn in legs:
                us[name].append(block_us(fn, inner[name]))
        return {k: statistics.median(v) for k, v in us.items()}, inner

    Kd, Cout, B = args.k, args.cout, args.anchors
    assert Cout % B == 0
    Cn = Cout // B - 5
    S = int(round(args.cells ** 0.5))
    assert S * S == args.cells
    rng = np.random.default_rng(0)
    Wt = (rng.standard_normal((Kd, Cout), np.float32) * np.float32(0.05))
    tree = E.WordTreeTables(generated_tree(Cn, args.depth))
    anchors = torch.as_tensor(np.asarray(((0.77871, 1.14074), (3.00525, 4.31277), (9.22725, 9.61974))[:B], np.float32)).cuda()
    thresh, iou, max_out = 0.005, 0.45, 100
    say("Detection on a word-tree head, K = %d -> %d (%d anchors x (5 + %d nodes in %d groups, depth %d)), S = %d; score_thresh "
        "%.3f, iou_thresh %.2f, max_out %d; HIP events, median of %d alternating blocks of %d calls, microseconds per call"
        % (Kd, Cout, B, Cn, tree.groups, tree.max_depth, S, thresh, iou, max_out, args.reps, args.inner))
    say("head      n  pass    (c) head  (d) detect  (c') top -1  (c') top %.3f  (d') tree detect  (f) one class  "
        "(c)+(d)  (c')+(d')  ratio  (d')/(f)" % thresh)
    for kind, to_bias in (("random", 0.0), ("trained", -8.0)):
        bias = rng.standard_normal(Cout, np.float32) * np.float32(0.5)
        bias.reshape(B, 5 + Cn)[:, 4] += np.float32(to_bias)
        wide = E.WideHead(Kd, Cout)
        wide.load(Wt, bias)
        for n in [int(v) for v in args.batches.split(",")]:
            x = torch.from_numpy(rng.standard_normal((n * args.cells, Kd), np.float32)).cuda()
            raw = wide.forward(x).view(n, S, S, B, 5 + Cn)
            head = torch.empty_like(raw)
            one = torch.zeros((n, S, S, B, 6), dtype=torch.float32, device="cuda")
            one[..., :5] = raw[..., :5]
            table = torch.from_numpy(np.array([(0, 375, 500, 1504, 0)] * n, np.int64)).cuda()
            outs = [(torch.empty((n, max_out, 6), dtype=torch.int32, device="cuda"),
                     torch.empty((n, max_out), dtype=torch.float32, device="cuda"),
                     torch.empty((n,), dtype=torch.int32, device="cuda")) for _ in range(3)]
            tops = [(torch.empty(raw.numel() // (5 + Cn), dtype=torch.int32, device="cuda"),
                     torch.empty(raw.numel() // (5 + Cn), dtype=torch.float32, device="cuda")) for _ in range(2)]

            def c():
                E.word_tree_head(raw, tree, 0.5, out=head)

            def d():
                E.detect_anchor_batch(head, anchors, table, None, thresh, iou, max_out, out=outs[0])

            def c1_all():
                E.word_tree_top(raw, tree, 0.5, None, out=tops[0])

            def c1():
                E.word_tree_top(raw, tree, 0.5, thresh, out=tops[1])

            def d1():
                E.detect_anchor_tree_batch(raw, tops[1][0], anchors, table, None, thresh, iou, max_out, out=outs[1])

            def f():
                E.detect_anchor_batch(one, anchors, table, None, thresh, iou, max_out, out=outs[2])

            c()
            c1()                             # (d) reads (c)'s rows, (d') reads (c')'s top
            med, inner = medians([("c", c), ("d", d), ("c1_all", c1_all), ("c1", c1), ("d1", d1), ("f", f)])
            torch.cuda.synchronize()
            for old, new in zip(outs[0], outs[1]):                       # faster and different is not faster
                assert torch.equal(old.view(torch.int32), new.view(torch.int32)), "(d') differs from (d)"
            share = (tops[1][0] >= 0).float().mean().item()
            before, after = med["c"] + med["d"], med["c1"] + med["d1"]
            say("%-7s  %2d  %4.2f  %10.1f  %10.1f  %11.1f  %13.1f  %16.1f  %13.1f  %7.1f  %9.1f  %5.1f  %8.2f%s"
                % (kind, n, share, med["c"], med["d"], med["c1_all"], med["c1"], med["d1"], med["f"], before, after,
                   before / after, med["d1"] / med["f"],
                   "".join("  [(%s): blocks of %d]" % (k, v) for k, v in sorted(inner.items()) if v != args.inner)))
            del x, raw, head, one, outs, tops
    say()
    say("pass: the share of the candidates whose objectness is > %.3f (the rows (c') at %.3f walks); ratio: ((c) + (d)) / "
        "((c') + (d')); the rows of (d') equal (d)'s bit for bit at every line" % (thresh, thresh))
    if args.out:
        with open(args.out, "w") as f_:
            f_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
