"""Same-box A/B of the MXFP8 inference mode (dtype "fp8") against f16 on the two forward-only workloads:

  configs[1]   darknet19_core forward, 416x416, batch 32, inference batch norm (bench.py --forward-only)
  classifier   darknet19 forward (core + 1x1 1024 -> 1000 + 7x7 average pool), 224x224, batch 128, inference batch norm

Variants: f16; fp8 (the product plan: net.hip mx8_layer admits only the shapes measured no slower); fp8-all (every
eligible shape on the MXFP8 kernel: Y2_MX8_ALL=1 at context creation) -- the per-layer f16 / fp8-all pairs are what the
plan's speed rule is read from.  Rounds alternate the variants (one network of each, built once); each round times `--steps` forwards after `--warmup`
untimed ones (wall clock over a synchronised loop, as bench.py).  Then per-layer milliseconds of one bracketed forward
per dtype (y2_profile_layers: every launch bracketed with HIP events, so the sum exceeds the loop time).  Prints one JSON
document; --out writes it too.

    python scripts/bench_fp8_infer.py --rounds 5 --steps 50 --warmup 10 --out profiles/fp8_infer_ab.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dtypes", default="f16,fp8-all,fp8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import torch
    from tensorflow_yolo2_amd import _lib, engine as E, synthetic

    workloads = [
        ("configs[1] core 416 b32", list(E.CORE_SPEC), 32, 416, _lib.Y2_TAIL_NONE),
        ("classifier 224 b128", list(E.CORE_SPEC) + list(E.CLS_HEAD_SPEC), 128, 224, _lib.Y2_TAIL_AVGPOOL),
    ]
    dtypes = args.dtypes.split(",")
    result = {"rounds": args.rounds, "steps": args.steps, "warmup": args.warmup, "workloads": []}
    for name, spec, bs, size, tail in workloads:
        x = torch.as_tensor(synthetic.images(bs, size, 1234)).cuda()
        nets = {}
        for dt in dtypes:
            if dt == "fp8-all":
                os.environ["Y2_MX8_ALL"] = "1"
            net = E.Network(spec, bs, size, size, dtype=dt.split("-")[0], core_layers=18, tail=tail, training=False)
            os.environ.pop("Y2_MX8_ALL", None)
            net.init_params(0)
            nets[dt] = net
        times = {dt: [] for dt in dtypes}
        for _ in range(args.rounds):
            for dt in dtypes:
                net = nets[dt]
                for _ in range(args.warmup):
                    net.forward(x, False, False)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    net.forward(x, False, False)
                torch.cuda.synchronize()
                times[dt].append((time.perf_counter() - t0) / args.steps * 1e3)
        layers = {}
        for dt in dtypes:
            net = nets[dt]
            net.forward(x, False, False)
            torch.cuda.synchronize()
            net.profile_enable(1)
            net.forward(x, False, False)
            torch.cuda.synchronize()
            per = net.profile_layers()
            net.profile_collect()
            net.profile_enable(0)
            layers[dt] = [round(float(v), 4) for v in per.sum(axis=1)]
        entry = {"workload": name, "batch": bs, "image_size": size,
                 "ms_per_forward": {dt: {"median": statistics.median(v), "min": min(v), "max": max(v),
                                         "rounds": [round(t, 4) for t in v]} for dt, v in times.items()},
                 "layer_ms": {"spec": [list(s) for s in spec], **layers}}
        result["workloads"].append(entry)
        print("%s: " % name + ", ".join("%s %.3f ms (%.3f..%.3f)" % (dt, statistics.median(v), min(v), max(v))
                                       for dt, v in times.items()), flush=True)
        del nets
        torch.cuda.empty_cache()
    doc = json.dumps(result, indent=1)
    print(doc)
    if args.out:
        with open(args.out, "w") as f:
            f.write(doc + "\n")


if __name__ == "__main__":
    main()
