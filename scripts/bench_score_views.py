"""What the classifier scoring costs (y2_score_views of csrc/score.hip, img_dataset/device_cls.DeviceCls.eval_views):

  kernel    microseconds of y2_score_views at (n, V, C) = (50, 10, 1000) and (128, 1, 1000) with labels, prob, rank and
            hits asked for -- in its two forms, the logits staged in LDS and re-read from L2 (Y2_SCORE_NO_STAGE=1) -- next
            to the chain of torch launches the predict script's host-side top-5 stands on: softmax -> view -> mean ->
            topk, plus the rank count, on the same logits.  HIP events around each call, blocks of calls alternate between
            the variants after a warm-up, median over all blocks.
  loop      the validation loop of imagenet_test_darknet.py per image at batch 50, f16: eval_views -> forward ->
            score_views, with --views stretch and with --views centre on a seeded list of 500 x 375 / 375 x 500 images;
            alternating blocks, HIP events around every batch, median.

    python scripts/bench_score_views.py --out profiles/score_views.txt
"""
import argparse
import os
import statistics
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_device_cls import make_list  # noqa: E402
from bench_device_voc import event_us  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="50x10x1000,128x1x1000", help="n x V x C, comma separated")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=5, help="alternating blocks per variant")
    ap.add_argument("--reps", type=int, default=40, help="timed calls per block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--images", type=int, default=100, help="images of the loop's list")
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import engine as E
    assert torch.cuda.is_available(), "needs the MI355X"
    lines = []

    def say(text=""):
        print(text, flush=True)
        lines.append(text)

    say("y2_score_views, k = %d, labels + prob + rank + hits; median of %d x %d calls per variant, alternating blocks, "
        "HIP events" % (args.k, args.blocks, args.reps))
    say("    n   V     C  reread_us  staged_us  torch_chain_us  torch/reread  staged/reread")
    for shape in args.shapes.split(","):
        n, V, Cn = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng([1, n, V, Cn])
        x = torch.from_numpy(np.float32(3 * rng.standard_normal((n * V, Cn)))).cuda()
        lab = torch.from_numpy(rng.integers(0, Cn, n).astype(np.int32)).cuda()
        lab64 = lab.long()
        outs = E.score_views(x, lab, views=V, k=args.k, want_prob=True)
        keep = dict(top_idx=outs[0], top_val=outs[1], rank=outs[2], hits=outs[3], prob=outs[4])

        def kernel():
            E.score_views(x, lab, views=V, k=args.k, **keep)

        def form(name):                         # the A/B switch is read at every call: set once per block
            os.environ.pop("Y2_SCORE_NO_STAGE", None)
            if name == "reread":
                os.environ["Y2_SCORE_NO_STAGE"] = "1"

        def chain():
            p = torch.softmax(x, dim=1).view(n, V, Cn).mean(dim=1)
            val, idx = torch.topk(p, args.k, dim=1)
            rank = (p > p.gather(1, lab64[:, None])).sum(dim=1)
            return val, idx, rank, (rank == 0).sum(), (rank < args.k).sum()

        calls = {"reread": kernel, "staged": kernel, "torch": chain}
        times = {name: [] for name in calls}
        for name, fn in calls.items():
            form(name)
            event_us(fn, args.warmup, 0)
        for _ in range(args.blocks):
            for name, fn in calls.items():
                form(name)
                times[name] += event_us(fn, 2, args.reps)
        os.environ.pop("Y2_SCORE_NO_STAGE", None)
        t = {name: statistics.median(v) for name, v in times.items()}
        say("%5d  %2d  %4d  %9.1f  %9.1f  %14.1f  %12.2f  %13.2f"
            % (n, V, Cn, t["reread"], t["staged"], t["torch"], t["torch"] / t["reread"], t["staged"] / t["reread"]))
    if not args.skip_loop:
        from tensorflow_yolo2_amd.img_dataset.device_cls import DeviceCls
        size, batch = 224, args.batch
        with tempfile.TemporaryDirectory() as tmp:
            items = make_list(tmp, args.images, seed=0)
            pool = DeviceCls(items, batch)
        net = E.Network(list(E.CORE_SPEC) + list(E.CLS_HEAD_SPEC), batch, size, size, dtype="f16",
                        core_layers=len(E.CORE_SPEC) + len(E.CLS_HEAD_SPEC), tail=E._lib.Y2_TAIL_AVGPOOL,
                        tail_k=size // 32, training=False)
        net.init_params(0)
        hits = torch.zeros(4, dtype=torch.int32, device="cuda")
        ranks = torch.empty(batch, dtype=torch.int32, device="cuda")
        starts = list(range(0, len(items), batch))
        cursor = [0]

        def loop(views):
            def f():
                start = starts[cursor[0] % len(starts)]
                cursor[0] += 1
                images, valid = pool.eval_views(size, start, views)
                labels = pool.labels_of(start)
                logits = net.forward(images, False, False)
                E.score_views(logits, labels, views=1, k=args.k, n_valid=valid, hits=hits, rank=ranks)
            return f

        calls = {"stretch": loop("stretch"), "centre": loop("centre")}
        times = {name: [] for name in calls}
        for fn in calls.values():
            event_us(fn, args.warmup, 0)
        for _ in range(args.blocks):
            for name, fn in calls.items():
                times[name] += event_us(fn, 1, args.reps // 2)
        t = {name: statistics.median(v) for name, v in times.items()}
        say()
        say("validation loop, f16 Darknet-19 at %d x %d, batch %d, %d images of 500 x 375 / 375 x 500: eval_views -> forward "
            "-> score_views" % (size, size, batch, len(items)))
        say("(median of %d x %d batches per variant, alternating blocks, HIP events around a batch)"
            % (args.blocks, args.reps // 2))
        say("views    batch_ms  per_image_us  centre/stretch")
        say("stretch  %8.3f  %12.1f" % (t["stretch"] / 1e3, t["stretch"] / batch))
        say("centre   %8.3f  %12.1f  %14.4f" % (t["centre"] / 1e3, t["centre"] / batch, t["centre"] / t["stretch"]))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
