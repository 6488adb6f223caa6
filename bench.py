#!/usr/bin/env python3
"""Headline benchmark: images/sec of the Darknet-19 YOLO detector TRAIN STEP
(darknet19_core + darknet19_detection + get_loss + backward + Adam) at 416x416,
batch 64 per GPU, synthetic inputs resident in HBM (BASELINE.json configs[3]; the
metric is quoted on fwd+bwd at 416x416, which fits one GPU).

    python bench.py --gpus N --steps K --warmup W            # the headline figure and nothing else
    python bench.py --gpus N --steps K --warmup W --full     # ... and every other leg described below
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Rank 0 prints ONE JSON line; `ms_per_step` is the wall time of one of the --steps timed steps.
A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line: `value`, `ms_per_step` and the
`roofline` of the timed region (its event brackets are part of the timed steps).  Everything that takes steps of its own
runs under `--full` only, after the timed region, and is then switched leg by leg with the --no-* / --*-steps options:
the serialised per-class pass (`kernels`), `sustained`, `fed_input`, the other BASELINE.json configurations
(`c1_detect`, `c2_forward`, `c3_classifier`, `c5_resnet50`), `f32_mode`, `parity_fast_mode*` and `cpu_baseline`.
`--dump-outputs DIR` writes what the last timed step returned (loss[5], ious, object mask; the forward output with
--forward-only) and a fixed, seeded sample of the parameters it updated as DIR/<name>.npy (float32): the inputs are
seeded, so two builds run with the same arguments can be compared output for output.
`roofline` is for the dominant kernel (the MFMA
implicit-GEMM convolution: forward, dgrad and wgrad launches): algorithmic FLOPs of those
launches / the union of their HIP-event intervals, measured on the launch streams inside the timed region.
`cpu_baseline` (--full) is the oracle's PyTorch-CPU restatement of the same train step on a
bounded sample (rank 0, N=1 only) -- "port", NOT the TF1 reference, which cannot run here.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MI355X_MICROARCH.md, dense.  "f16x2" (split-operand mode: three f16 MFMAs per product) is priced against the f16
# peak with the ALGORITHMIC FLOPs counted once -- its own ceiling is a third of that, 833 TFLOP/s
MFMA_PEAK_TFLOPS = {"f16": 2500.0, "bf16": 2500.0, "f32": 157.3, "f16x2": 2500.0, "f16x2f": 2500.0}


def conv_flops(spec, batch, size):
    """(forward FLOPs of the implicit-GEMM layers, of conv1, list per layer)"""
    h = size
    per = []
    for (k, ci, co, pool) in spec:
        per.append(2.0 * batch * h * h * k * k * ci * co)
        if pool:
            h = (h + 1) // 2
    return per


def usable_cores():
    """cores this process may really use: affinity mask capped by the cgroup CPU quota"""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def core_counts():
    """(physical cores, logical CPUs) of the host, from /proc/cpuinfo"""
    logical = os.cpu_count() or 1
    phys = set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("physical id"):
                pid = line.split(":")[1].strip()
            elif line.startswith("core id"):
                cid = line.split(":")[1].strip()
            elif not line.strip():
                if pid is not None and cid is not None:
                    phys.add((pid, cid))
                pid = cid = None
        if pid is not None and cid is not None:
            phys.add((pid, cid))
    except OSError:
        pass
    return (len(phys) or logical), logical


def spawn_ranks(args):
    """`python bench.py --gpus N` outside torchrun: start the N ranks ourselves, as a CHILD process tree,
    before this process has touched the GPU (no HIP call yet; never exec from a GPU-initialised process),
    and leave with its exit code.  Rank 0 of the children prints the JSON line."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    return subprocess.call(cmd, env=env)


def cpu_baseline(args, spec_core, spec_head):
    """oracle (torch-CPU restatement) timed on the host cores: bounded sample of the same workload."""
    import numpy as np
    import torch
    from oracle import torch_ref as T, nn_ref as R
    from tensorflow_yolo2_amd import synthetic
    cores = usable_cores()
    torch.set_num_threads(cores)
    bs = args.cpu_batch
    size, S = args.image_size, args.image_size // 32
    spec = [(k, ci, co, bool(p)) for (k, ci, co, p) in spec_core + spec_head]
    params = T.to_torch_params(R.init_params(spec, seed=0), torch.float32, requires_grad=True)
    step = T.detector_train_step_fn(spec[:len(spec_core)], spec[len(spec_core):], params, S, 2, 20, size)
    x = torch.as_tensor(synthetic.images(bs, size, 1234))
    lab = torch.as_tensor(synthetic.det_labels(bs, size, S, 4321))
    step(x, lab)                                   # warm-up
    times = []
    t_end = time.time() + args.cpu_seconds
    while len(times) < 5 and (time.time() < t_end or not times):
        t0 = time.time()
        step(x, lab)
        times.append(time.time() - t0)
    med = sorted(times)[len(times) // 2]
    phys, logical = core_counts()
    return {"value": bs / med, "unit": "images/s", "cores": cores, "physical_cores": phys, "logical_cpus": logical,
            "kind": "port",
            "sample": "oracle/torch_ref.py (PyTorch-CPU fp32 restatement, not TF1): detector fwd+loss+bwd, "
                      "%dx%d, batch %d, median of %d steps, %d threads" % (size, size, bs, len(times), cores)}


def f32_mode(args, images, labels, device, total_flops, igemm_flops, dtype="f32"):
    """the parity-grade arithmetic timed on the same workload -- dtype "f32": exact-f32 MFMA, the mode the 1e-3 tests
    gate; dtype "f16x2" (the `parity_fast_mode` leg, round 5): the same end-to-end tolerance on the f16 matrix pipe,
    split operands, three MFMAs per product -- 2 warm-up + --f32-steps timed steps bracketed like the headline run,
    with its own roofline sub-record (MFMA convolution launches, union of their HIP-event intervals on every 4th
    step, against the dense peak of the pipe it runs on, algorithmic FLOPs counted once)"""
    import torch
    from tensorflow_yolo2_amd.trainer import DetectorTrainer
    tr = DetectorTrainer(args.batch, args.image_size, dtype=dtype, device=device, seed=0)
    for _ in range(2):
        tr.step(images, labels)
    torch.cuda.synchronize()
    n = max(1, args.f32_steps)
    sampled = 0
    t0 = time.perf_counter()
    for i in range(n):
        if i % 4 == 0:
            tr.net.profile_enable(2 if sampled == 0 else 3)
            sampled += 1
        elif i % 4 == 1:
            tr.net.profile_enable(0)
        tr.step(images, labels)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    busy_ms, launches = tr.net.profile_busy()
    tr.net.profile_collect()
    tr.net.profile_enable(0)
    peak = MFMA_PEAK_TFLOPS[dtype]
    tf = total_flops / (ms * 1e-3) / 1e12
    out = {"dtype": dtype, "ms_per_step": ms, "images_per_s": args.batch / (ms * 1e-3), "steps": n, "warmup": 2,
           "whole_step_tflops": tf, "peak": peak, "whole_step_frac": tf / peak}
    if busy_ms > 0 and sampled:
        t = busy_ms / sampled * 1e-3
        out["roofline"] = {"bound": "mfma", "achieved": igemm_flops / t / 1e12, "peak": peak, "unit": "TFLOP/s",
                           "frac": igemm_flops / t / 1e12 / peak, "avg_launch_ms": busy_ms / max(launches, 1),
                           "launches_per_step": launches / sampled, "bracketed_steps": sampled,
                           "kernel": ("MFMA implicit-GEMM convolution launches in exact-f32 MFMA (v_mfma_f32_32x32x2_f32)"
                                      if dtype == "f32" else
                                      "MFMA implicit-GEMM convolution launches, split operands: hi*hi + lo*hi + hi*lo on "
                                      "v_mfma_f32_*_f16, fp32 accumulate; FLOPs counted once")}
    if dtype == "f16x2":
        out["mfma_issued_frac"] = 3.0 * out["roofline"]["frac"] if "roofline" in out else None
        out["note"] = ("reference-tolerance mode on the fast matrix pipe: end to end within 1e-3 of the fp32 reference "
                       "(tests/test_gpu_f16x2.py); frac = algorithmic FLOPs / 2.5 PF, the pipe issues three times that")
    if dtype == "f16x2f":
        # forward: three products per MAC; dgrad and weight gradients: one (hi planes) -- 5/3 of the algorithmic FLOPs issued
        out["mfma_issued_frac"] = 5.0 / 3.0 * out["roofline"]["frac"] if "roofline" in out else None
        out["note"] = ("round 6: f16x2 forward (split operands, every forward decision at reference precision) + backward "
                       "contractions on the hi planes only (one f16 MFMA per product); the whole-step gates of the exact-f32 "
                       "mode hold unchanged (tests/test_gpu_f16x2f.py); frac = algorithmic FLOPs / 2.5 PF")
    # per-class table: a serialised, untimed pass that brackets every launch
    tr.net.profile_enable(1)
    for _ in range(3):
        tr.step(images, labels)
    torch.cuda.synchronize()
    out["kernels"] = {k: {"ms_per_step": v[0] / 3, "launches_per_step": v[1] / 3} for k, v in tr.net.profile_collect().items()}
    tr.net.profile_enable(0)
    return out


def sustained(run, sync_all, steps, batch, world):
    """a second, longer timed region (no events): the clock the chip holds once DVFS and temperature have settled"""
    sync_all()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    sync_all()
    el = time.perf_counter() - t0
    return {"steps": steps, "ms_per_step": el / steps * 1e3, "images_per_s": world * batch * steps / el}


def dump_outputs(dirname, arrays):
    """--dump-outputs: one DIR/<name>.npy per array (float32, or float64 where the array is float64), at most 64 MB"""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    total = 0
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        a = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
        total += a.nbytes
        assert total <= 64 << 20, "--dump-outputs: more than 64 MB"
        np.save(os.path.join(dirname, name + ".npy"), a)


def param_sample(params, k=1 << 20, seed=0):
    """a fixed, seeded sample of k entries of a flat parameter buffer (sorted indices, the same for every run)"""
    import numpy as np
    import torch
    n = params.numel()
    if n <= k:
        return params
    idx = np.sort(np.random.default_rng(seed).choice(n, k, replace=False))
    return params[torch.as_tensor(idx, device=params.device)]


def extra_leg(name, net, run, spec, flop_mult, bs, size, dtype, steps=20, warmup=3):
    """another BASELINE.json configuration timed in the same process (driver-visible: the driver only runs
    `bench.py --gpus 1`): `warmup` untimed + `steps` timed steps between synchronisations; the MFMA convolution
    launches of two of them are bracketed with HIP events (union of the intervals, as the headline's `roofline.frac`)"""
    import torch
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    sampled = 0
    t0 = time.perf_counter()
    for i in range(steps):
        if i % 10 == 0:
            net.profile_enable(2 if sampled == 0 else 3)
            sampled += 1
        elif i % 10 == 1:
            net.profile_enable(0)
        run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    busy_ms, launches = net.profile_busy()
    net.profile_collect()
    net.profile_enable(0)
    per = conv_flops(spec, bs, size)
    total, igemm = sum(per) * flop_mult, sum(per[1:]) * flop_mult
    peak = MFMA_PEAK_TFLOPS[dtype]
    out = {"workload": name, "dtype": dtype, "batch": bs, "image_size": size, "steps": steps, "warmup": warmup,
           "ms_per_step": ms, "images_per_s": bs / (ms * 1e-3), "whole_step_tflops": total / (ms * 1e-3) / 1e12,
           "whole_step_frac": total / (ms * 1e-3) / 1e12 / peak, "frac": None}
    if busy_ms > 0 and sampled:
        t = busy_ms / sampled * 1e-3
        out.update({"frac": igemm / t / 1e12 / peak, "mfma_launch_union_ms": busy_ms / sampled,
                    "launches_per_step": launches / sampled, "bracketed_steps": sampled})
    return out


def c2_forward_leg(args, device):
    """BASELINE.json configs[1]: darknet19_core forward, 416x416, batch 32, batch norm with the moving statistics
    (pascal_detect_darknet.py:41-43)"""
    import torch
    from tensorflow_yolo2_amd import engine as E, synthetic
    bs, size = 32, 416
    net = E.Network(list(E.CORE_SPEC), bs, size, size, dtype=args.dtype, training=False, device=device)
    net.init_params(0)
    x = torch.as_tensor(synthetic.images(bs, size, 1234)).to(device)
    out = extra_leg("configs[1]: darknet19_core forward 416x416 batch 32, inference batch norm", net,
                    lambda: net.forward(x, False, False), list(E.CORE_SPEC), 1.0, bs, size, args.dtype)
    out["target_ms"] = 0.65                      # 40 % of the dense peak
    return out


def c1_detect_leg(args, device):
    """BASELINE.json configs[0]: pascal_detect_darknet.py's graph -- core with the moving statistics, head with its
    default batch statistics (pascal_detect_darknet.py:41-43), ONE 224x224 image -- as a serving latency: host call ->
    result on the host side of a synchronisation, eager launches against one HIP-graph replay (engine.ForwardGraph)"""
    import torch
    from tensorflow_yolo2_amd import engine as E, synthetic
    size = 224
    spec = list(E.CORE_SPEC) + E.det_head_spec(30)
    net = E.Network(spec, 1, size, size, dtype=args.dtype, core_layers=len(E.CORE_SPEC), training=False, device=device)
    net.init_params(0)
    x = torch.as_tensor(synthetic.images(1, size, 1234)).to(device)
    n = 200

    def timed(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
            torch.cuda.synchronize()           # the detection is consumed on the host: latency, not throughput
        return (time.perf_counter() - t0) / n * 1e3
    eager = timed(lambda: net.forward(x, False, True))
    ref = net.forward(x, False, True).clone()
    g = net.forward_graph(False, True)
    g.input.copy_(x)
    graph = timed(g.replay)
    torch.cuda.synchronize()
    # bit patterns: an UNTRAINED network in inference mode (moving statistics 0 / 1) overflows f16 towards the top, and
    # NaN != NaN under torch.equal
    same = bool(torch.equal(g.output.view(torch.int32), ref.view(torch.int32)))
    per = conv_flops(spec, 1, size)
    return {"workload": "configs[0]: single-image detection forward 224x224 (core inference BN + head batch statistics)",
            "dtype": args.dtype, "batch": 1, "image_size": size, "images": n,
            "eager_ms_per_image": eager, "graph_ms_per_image": graph, "graph_speedup": eager / graph,
            "graph_output_equals_eager": same, "gflop_per_image": sum(per) / 1e9,
            "note": "GPU-bound, not launch-bound: at batch 1 a 13x13-class layer is 8 workgroups streaming 19-38 MB of "
                    "filters (one pixel tile x 8 cout tiles); the graph replay removes ~40 host launches and changes "
                    "little -- a weight-streaming small-M convolution form is what this configuration wants"}


def c3_classifier_leg(args, device):
    """BASELINE.json configs[2]: darknet19() + softmax cross-entropy fwd+bwd + Momentum(0.001, 0.9), 224x224, batch 128
    (src/imagenet/imagenet_train_darknet.py:46-58)"""
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.trainer import ClassifierTrainer
    bs, size = 128, 224
    tr = ClassifierTrainer(bs, size, dtype=args.dtype, device=device, seed=0)
    x = torch.as_tensor(synthetic.images(bs, size, 1234)).to(device)
    lab = torch.as_tensor(np.random.default_rng(5).integers(0, 1000, bs).astype(np.int32)).to(device)
    out = extra_leg("configs[2]: darknet19 classifier fwd+bwd + Momentum 224x224 batch 128", tr.net,
                    lambda: tr.step(x, lab), list(E.CORE_SPEC) + list(E.CLS_HEAD_SPEC), 3.0, bs, size, args.dtype)
    out["target_ms"] = 2.30
    return out


def _resnet_settle(m, x, lab, want=3, limit=60):
    """run steps until `want` consecutive ones were APPLIED (the f16 loss scaler halves its scale after an overflowing step
    and the guarded optimizer skips that step on the device: a skipped step does not run the 1.64 GB Adam update of
    yolo_fc1 and is ~2 ms shorter -- round 5 found the graph leg timing skipped steps, because the graph follows the
    control block only every graph_check_every steps).  During the settling the control block is followed every step."""
    import torch
    every = m.graph_check_every
    m.graph_check_every = 1
    run = 0
    for _ in range(limit):
        before = int(m.ctrl[1])
        m.step(x, lab)
        torch.cuda.synchronize()
        run = run + 1 if int(m.ctrl[1]) == before + 1 else 0
        if run >= want:
            break
    m.graph_check_every = every
    if m.graph:
        m.step(x, lab)          # (a changed scale re-captures: keep the capture out of the timed region)
        m.step(x, lab)
        torch.cuda.synchronize()
    return run >= want


def _resnet_timed(m, x, lab, n):
    """n steps, timed; returns (ms per step, steps applied, steps skipped) from the device control block"""
    import torch
    torch.cuda.synchronize()
    a0, s0 = int(m.ctrl[1]), int(m.ctrl[2])
    t0 = time.perf_counter()
    for _ in range(n):
        m.step(x, lab)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    return ms, int(m.ctrl[1]) - a0, int(m.ctrl[2]) - s0


def c5_resnet50_leg(args, device):
    """BASELINE.json configs[4], second half: the reference's ResNet-50 backbone swap (slim resnet_v1_50 + the YOLO FC
    head, src/pascal/pascal_train_resnet.py:37-50) -- one train step at batch 32, 224x224, replayed from ONE HIP graph
    (forward, loss, backward, overflow scan, guarded Adam); the stride-1 bottleneck units run on the native stack executor"""
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.yolo2_nets.tf_resnet import ResNet50Yolo
    bs, size = 32, 224
    # (the ResNet swap has no split-operand form: under --dtype f16x2 / f16x2f this leg runs its f16 arithmetic)
    rdtype = "f16" if args.dtype in ("f16x2", "f16x2f") else args.dtype
    m = ResNet50Yolo(bs, size, dtype=rdtype, device=device, seed=0, graph=True)
    x = torch.as_tensor(synthetic.images(bs, size, 1234)).to(device)
    lab = torch.as_tensor(synthetic.det_labels(bs, size, size // 32, 4321)).to(device)
    for _ in range(4):                      # two eager steps, the capture, one replay
        m.step(x, lab)
    torch.cuda.synchronize()
    # the loss scale has adapted: the timed steps are APPLIED steps.  (An unguarded f32 model has no control block to
    # follow -- the host counts its steps -- so there is nothing to settle and every step is applied: ADVICE r5)
    settled = _resnet_settle(m, x, lab) if m.guard else True
    n = 10
    ms, applied, skipped = _resnet_timed(m, x, lab, n)
    if not m.guard:
        applied, skipped = n, 0
    if skipped:                             # an overflow inside the timed region: settle again, time again
        settled = _resnet_settle(m, x, lab)
        ms, applied, skipped = _resnet_timed(m, x, lab, n)
    flops = m.flops_per_step()
    return {"workload": "configs[4]: ResNet-50 backbone swap train step 224x224 batch 32 (HIP-graph replay)", "dtype": rdtype,
            "batch": bs, "image_size": size, "steps": n, "warmup": 4, "ms_per_step": ms, "images_per_s": bs / (ms * 1e-3),
            "steps_applied": applied, "steps_skipped_by_overflow_guard": skipped, "loss_scale": m.loss_scale,
            "loss_scale_settled": bool(settled),
            "whole_step_tflops": flops / (ms * 1e-3) / 1e12,
            "whole_step_frac": flops / (ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[rdtype], "fused_stacks": bool(m.fused)}


def fed_input(args, tr, device, resident_ms):
    """the fed loop: uint8 batches assembled in pinned memory and uploaded on their own stream while the previous
    step runs (utils/feeder.py), the float conversion inside the input pack kernel (y2_forward_u8).  The producer
    copies pre-decoded uint8 images out of a host pool (what img_dataset.pascal_voc.get_u8 does with its cache)."""
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.utils.feeder import DeviceFeeder
    bs, size, S = args.batch, args.image_size, args.image_size // 32
    rng = np.random.default_rng(7)
    pool = rng.integers(0, 256, (4 * bs, size, size, 3), dtype=np.uint8)
    labs = synthetic.det_labels(4 * bs, size, S, 99)
    state = {"k": 0}

    def produce(im, lab):
        k = state["k"] % 4
        im[...] = pool[k * bs:(k + 1) * bs]
        lab[...] = labs[k * bs:(k + 1) * bs]
        state["k"] += 1
    feeder = DeviceFeeder(produce, bs, size, S, device=device)
    n = max(1, args.fed_steps)

    def one():
        img, lab = feeder.get()
        tr.step(img, lab)
        feeder.release()
        feeder.prefetch()
    for _ in range(3):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        one()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    return {"steps": n, "ms_per_step": ms, "images_per_s": bs / (ms * 1e-3), "vs_resident_input": ms / resident_ms,
            "upload_bytes_per_step": bs * size * size * 3 + bs * S * S * 25 * 4,
            "path": "pinned double buffer -> upload stream (uint8, 1 B per value) -> y2_forward_u8"}


def bench_yolov2(args, images, labels, device, rank, world, dist):
    """train step of the YOLOv2 anchor model (yolo2_nets/yolov2.py): same contract, its own metric name"""
    import torch
    from tensorflow_yolo2_amd.yolo2_nets.yolov2 import YOLOv2Trainer
    tr = YOLOv2Trainer(args.batch, args.image_size, dtype=args.dtype, device=device, seed=0)

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
    for _ in range(args.warmup):
        tr.step(images, labels)
    sync_all()
    nets = tr.networks()
    stride, sampled = max(1, args.event_stride), 0
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.kernel_events == "timed":
            if i % stride == 0:
                for nt in nets:
                    nt.profile_enable(2 if sampled == 0 else 3)
                sampled += 1
            elif i % stride == 1 or stride == 1:
                for nt in nets:
                    nt.profile_enable(0)
        tr.step(images, labels)
    sync_all()
    elapsed = time.perf_counter() - t0
    # the three stacks run one after the other (each y2_backward joins its side stream before it returns), so the
    # union of all MFMA launch intervals is the sum of the three stacks' unions
    busy_ms, launches = 0.0, 0
    if args.kernel_events == "timed":
        for nt in nets:
            b = nt.profile_busy()
            busy_ms += b[0]
            launches += b[1]
            nt.profile_collect()
            nt.profile_enable(0)
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    out = None
    if rank == 0:
        ms = elapsed / args.steps * 1e3
        flops = tr.flops_per_step()
        peak = MFMA_PEAK_TFLOPS[args.dtype]
        roof = {"bound": "mfma", "achieved": None, "peak": peak, "unit": "TFLOP/s", "frac": None, "traffic": None,
                "kernel": "MFMA implicit-GEMM convolution launches of the three stacks (forward, dgrad, wgrad); time = "
                          "union of the launch intervals", "whole_step_frac": flops / (ms * 1e-3) / 1e12 / peak}
        if busy_ms > 0 and sampled:
            t_ig = busy_ms / sampled * 1e-3
            ig = tr.flops_per_step(mfma_launches_only=True)
            roof.update({"achieved": ig / t_ig / 1e12, "frac": ig / t_ig / 1e12 / peak,
                         "avg_launch_ms": busy_ms / max(launches, 1), "launches_per_step": launches / sampled,
                         "bracketed_steps": sampled, "flops_per_launch": ig / max(launches / sampled, 1)})
        out = {"metric": "images/sec fwd+bwd YOLOv2 (Darknet-19 + passthrough + anchor loss) 416x416",
               "value": world * args.batch * args.steps / elapsed, "unit": "images/s", "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
               "scaling": "weak", "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
               "config": {"workload": "YOLOv2 train step: stem (13 layers) + pool + 13x13 stack (7 layers) + passthrough "
                                      "concat 3072 + head (3x3, 1x1 -> 125) + anchor loss + backward + Adam "
                                      "(north-star model, not in the reference)",
                          "image_size": args.image_size, "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                          "S": args.image_size // 32, "B": tr.B, "parallelism": "dp%d" % world},
               "whole_step_tflops": flops / (ms * 1e-3) / 1e12,
               "roofline": roof}
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out


def bench_resnet(args, device, rank, world, dist):
    """train step of the ResNet-50 backbone swap (yolo2_nets/tf_resnet.py; BASELINE.json configs[4]; the reference trains
    it at batch 4, 224x224: src/pascal/pascal_train_resnet.py:26).  An operator-level composition, not a tuned path:
    the roofline is the whole step's algorithmic FLOPs over wall time."""
    import torch
    from tensorflow_yolo2_amd import synthetic
    from tensorflow_yolo2_amd.yolo2_nets.tf_resnet import ResNet50Yolo
    bs, size = args.batch, 224
    dtype = args.dtype
    m = ResNet50Yolo(bs, size, dtype=dtype, device=device, seed=0, graph=args.graph)
    x = torch.as_tensor(synthetic.images(bs, size, 1234 + rank)).to(device)
    lab = torch.as_tensor(synthetic.det_labels(bs, size, size // 32, 4321 + rank)).to(device)
    for _ in range(max(args.warmup, 4) if args.graph else args.warmup):     # graph: two eager steps, capture, one replay
        m.step(x, lab)
    torch.cuda.synchronize()
    settled = _resnet_settle(m, x, lab) if m.guard else True

    def timed():
        # replicas: barrier + synchronize on both sides, the slowest rank's clock (the contract of the headline line)
        if dist is not None:
            torch.cuda.synchronize()
            dist.barrier()
        ms_, applied_, skipped_ = _resnet_timed(m, x, lab, args.steps)
        if dist is not None:
            t = torch.tensor([ms_], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ms_ = float(t.item())
        return ms_, applied_, skipped_

    ms, applied, skipped = timed()
    if not m.guard:
        applied, skipped = args.steps, 0
    if skipped:                 # (the control block is identical on every replica: all of them take this branch or none)
        settled = _resnet_settle(m, x, lab)
        ms, applied, skipped = timed()
    flops = m.flops_per_step() * world
    peak = MFMA_PEAK_TFLOPS[dtype] * world
    out = {"metric": "images/sec fwd+bwd ResNet-50 (slim resnet_v1_50 + YOLO FC head) 224x224", "value": world * bs / (ms * 1e-3),
           "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms,
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
           "config": {"workload": "ResNet-50 backbone swap train step: resnet_v1_50 (16 bottleneck units) + FC 4096 + dropout "
                                  "+ FC 1470 + get_loss + backward + Adam(0.0005)", "image_size": size, "batch_per_gpu": bs,
                      "global_batch": bs * world, "S": 7, "B": 2, "parallelism": "dp%d" % world,
                      "launch": "one HIP graph replay per step" if (args.graph and world == 1) else "per-operator launches from Python",
                      "grad_exchange": None if world == 1 else
                      {"flat_buffer": "SUM all-reduce of every gradient in front of yolo_fc1/weights (%.1f MB), strategy %s"
                                      % (m.offset["yolo_fc1/weights"][0] * 4 / 1e6 if m._fc1_fused_now() else m.params.numel() * 4 / 1e6,
                                         m.dp_strategy),
                       "yolo_fc1": ("all-gather of its operands x [%d, %d] and dz [%d, %d] per rank; every rank runs the fused "
                                    "product + guarded Adam over the %d gathered rows -- the %.2f GB gradient is never formed"
                                    % (bs, m.p["yolo_fc1/weights"].shape[0], bs, m.p["yolo_fc1/weights"].shape[1], bs * world,
                                       m.p["yolo_fc1/weights"].numel() * 4 / 1e9)) if m._fc1_fused_now() else
                                   "stored gradient inside the flat all-reduce (gathered batch beyond the fused kernel's 256 rows, or f32)"},
                      "note": "the stride-1 / stride-2 bottleneck units on the native stack executor; batch-norm statistics per replica"},
           "steps_applied": applied, "steps_skipped_by_overflow_guard": skipped, "loss_scale": m.loss_scale,
           "loss_scale_settled": bool(settled),
           "whole_step_tflops": flops / (ms * 1e-3) / 1e12,
           "roofline": {"bound": "mfma", "achieved": flops / (ms * 1e-3) / 1e12, "peak": peak, "unit": "TFLOP/s",
                        "frac": flops / (ms * 1e-3) / 1e12 / peak, "traffic": None,
                        "kernel": "whole step (convolution + FC FLOPs as defined / wall time): launch-bound at batch %d" % bs}}
    if rank == 0:
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=64, help="images per GPU")
    ap.add_argument("--image-size", type=int, default=416)
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "f32", "f16x2", "f16x2f"])
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every leg that takes steps of its own: per-class kernel pass, "
                         "sustained, fed input, the other configurations, f32 / parity modes, CPU baseline (the --no-* and "
                         "--*-steps options below choose among them); off: the headline figure only")
    ap.add_argument("--kernel-events", default="timed", choices=["timed", "separate", "off"],
                    help="timed: bracket the MFMA launches of every --event-stride-th timed step; separate (--full only): "
                         "no brackets in the timed steps, the serialised pass alone; off: none")
    ap.add_argument("--event-stride", type=int, default=10, help="bracket the MFMA launches of every n-th timed step")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-batch", type=int, default=8)     # bs 8
    ap.add_argument("--cpu-seconds", type=float, default=25.0)
    ap.add_argument("--no-f32-mode", action="store_true")
    ap.add_argument("--no-fast-parity-mode", action="store_true", help="skip the f16x2 (split-operand) leg")
    ap.add_argument("--f32-steps", type=int, default=12)
    ap.add_argument("--sustain-steps", type=int, default=300, help="extra timed region without events (0: skip)")
    ap.add_argument("--fed-steps", type=int, default=30, help="fed-input leg: uint8 upload pipeline (0: skip)")
    ap.add_argument("--forward-only", action="store_true", help="configs[1]: core forward only (inference BN)")
    ap.add_argument("--no-extra-legs", action="store_true",
                    help="skip the c1_detect (configs[0]), c2_forward (configs[1]), c3_classifier (configs[2]) and c5_resnet50 (configs[4]) legs of the default line")
    ap.add_argument("--model", default="detector", choices=["detector", "yolov2", "resnet50", "classifier"],
                    help="detector: the reference's Darknet-19 grid detector (the headline); yolov2: the north star's "
                         "anchor model (passthrough + anchor loss), not in the reference")
    ap.add_argument("--graph", action="store_true", help="resnet50: replay the step from one HIP graph")
    ap.add_argument("--own-stream", action="store_true", help="run on a torch side stream instead of the default (NULL) stream")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL, default) | gloo (single-GPU functional test)")
    ap.add_argument("--all-ranks-on-gpu0", action="store_true", help="functional test of the N>1 path on one GPU")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) to DIR/<name>.npy; --model detector only")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.model != "detector":
        ap.error("--dump-outputs: --model detector only")
    if args.kernel_events == "separate" and not args.full:
        ap.error("--kernel-events separate measures in a pass of its own: add --full")

    if args.gpus > 1 and "RANK" not in os.environ and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args))

    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E, synthetic
    from tensorflow_yolo2_amd.trainer import DetectorTrainer

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.all_ranks_on_gpu0:
            local_rank = 0
            # functional test only: two PROCESSES time-slicing one GPU, each with a side stream, stall on each
            # other's queue slices (measured 3 s per step); production is one process per GPU
            os.environ["Y2_NO_WGRAD_OVERLAP"] = "1"
            if args.dist_backend == "nccl":
                args.dist_backend = "gloo"      # RCCL refuses two ranks on one device
        torch.cuda.set_device(local_rank)
        if args.dist_backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(args.dist_backend, rank=rank, world_size=world)
    assert world == args.gpus, "launch with torch.distributed.run --nproc-per-node %d" % args.gpus
    device = "cuda:%d" % local_rank
    torch.cuda.set_device(device)
    if args.own_stream:
        torch.cuda.set_stream(torch.cuda.Stream(device=device))

    size, bs = args.image_size, args.batch
    S = size // 32
    spec_core, spec_head = list(E.CORE_SPEC), E.det_head_spec(30)
    images = torch.as_tensor(synthetic.images(bs, size, 1234 + rank)).to(device)
    labels = torch.as_tensor(synthetic.det_labels(bs, size, S, 4321 + rank)).to(device)

    if args.model == "yolov2":
        return bench_yolov2(args, images, labels, device, rank, world, dist)
    if args.model == "resnet50":
        if args.dtype in ("f16x2", "f16x2f"):
            sys.exit("--model resnet50: --dtype f32 | f16 | bf16 (the split-operand modes exist for the Darknet-19 stacks only)")
        return bench_resnet(args, device, rank, world, dist)
    if args.model == "classifier":      # configs[2] on its own (what profiles/r04_*_c3* trace)
        assert world == 1
        out = c3_classifier_leg(args, device)
        line = {"metric": "images/sec fwd+bwd Darknet-19 classifier 224x224", "value": out["images_per_s"],
                "unit": "images/s", "n_gpus": 1, "steps": out["steps"], "warmup": out["warmup"],
                "ms_per_step": out["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                "dtype": args.dtype, "data": "synthetic", "config": {"workload": out["workload"]},
                "roofline": {"bound": "mfma", "peak": MFMA_PEAK_TFLOPS[args.dtype], "unit": "TFLOP/s",
                             "frac": out["frac"], "whole_step_frac": out["whole_step_frac"], "traffic": None}}
        print(json.dumps(line))
        return line
    if args.forward_only:
        net = E.Network(spec_core, bs, size, size, dtype=args.dtype, training=False, device=device)
        net.init_params(0)
        run = lambda: net.forward(images, False, False)
        spec = spec_core
        flop_mult = 1.0
    else:
        tr = DetectorTrainer(bs, size, dtype=args.dtype, device=device, seed=0)
        net = tr.net
        run = lambda: tr.step(images, labels)
        spec = spec_core + spec_head
        flop_mult = 3.0

    def sync_all():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        run()
    sync_all()
    # timed region: HIP events bracket ONLY the dominant kernel's launches (the MFMA implicit-GEMM
    # convolutions: forward, dgrad and weight gradient, 63 of ~150 launches per step) so that the
    # measurement does not cost the step ~6 %.  The weight gradients run on a side stream beside the
    # dgrads, so the kernel time is the UNION of the launch intervals (y2_profile_busy), not their sum.
    # A second, untimed and serialised pass brackets every launch for the per-class table (--full).
    # Events cost ~3 us per bracketed launch (they break back-to-back dispatch), so only every
    # `--event-stride`-th step of the timed region is bracketed; the roofline uses those steps.
    stride = max(1, args.event_stride)
    sampled = 0
    # the guarded optimizer skips an overflowing step on the device (half-precision modes): count what the timed steps did
    scaler = getattr(getattr(tr, "opt", None), "scaler", None) if not args.forward_only else None
    st0 = scaler.state() if scaler is not None else None
    t0 = time.perf_counter()
    for i in range(args.steps):
        if args.kernel_events == "timed":
            if i % stride == 0:
                net.profile_enable(2 if sampled == 0 else 3)
                sampled += 1
            elif i % stride == 1 or stride == 1:
                net.profile_enable(0)
        last = run()
    sync_all()
    elapsed = time.perf_counter() - t0
    st1 = scaler.state() if scaler is not None else None
    if args.dump_outputs and rank == 0:
        # what a caller of the timed path received from its last step, taken before anything else runs on the network:
        # the train step's (loss[5], ious, object mask) and a sample of the parameters its Adam update wrote, or the
        # forward's output
        if args.forward_only:
            dump_outputs(args.dump_outputs, {"output": last})
        else:
            loss, ious, mask = last
            dump_outputs(args.dump_outputs, {"loss": loss, "ious": ious, "object_mask": mask,
                                             "params_sample": param_sample(net.params)})
    busy = net.profile_busy() if args.kernel_events == "timed" else None
    prof = net.profile_collect() if args.kernel_events == "timed" else None
    net.profile_enable(0)
    prof_all = None
    if args.full and args.kernel_events in ("timed", "separate"):
        net.profile_enable(1)
        for _ in range(args.steps):
            run()
        torch.cuda.synchronize()
        prof_all = net.profile_collect()
        net.profile_enable(0)
        if prof is None:
            prof = prof_all

    sus = sustained(run, sync_all, args.sustain_steps, bs, world) if args.full and args.sustain_steps > 0 else None
    if dist is not None:
        t = torch.tensor([elapsed] + ([sus["ms_per_step"]] if sus else []), dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t[0].item())
        if sus:
            sus["ms_per_step"] = float(t[1].item())
            sus["images_per_s"] = world * bs / (sus["ms_per_step"] * 1e-3)

    ms_per_step = elapsed / args.steps * 1e3
    value = world * bs * args.steps / elapsed

    out = None
    if rank == 0:
        per = conv_flops(spec, bs, size)
        fwd_igemm = sum(per[1:])
        # forward, dgrad and wgrad launches of layers 1..L-1 (the 3 -> 32 first layer has its own kernels)
        igemm_flops = fwd_igemm * (1.0 if args.forward_only else 3.0)
        roof = {"bound": "mfma", "achieved": None, "peak": MFMA_PEAK_TFLOPS[args.dtype], "unit": "TFLOP/s",
                "frac": None, "traffic": None, "kernel": "MFMA implicit-GEMM convolution: forward, dgrad and wgrad launches (conv_haloq / conv_halo / conv_igemm / conv_rf / wgrad9 / wgrad); time = union of the launch intervals"}
        kernels = None
        if prof is not None:
            if busy is not None and busy[1] > 0:      # the bracketed steps of the timed region
                psteps = max(sampled, 1)
                t_igemm, n_launch = busy[0] / psteps * 1e-3, busy[1]
            else:   # serialised pass: the sum of the durations is the busy time
                psteps = args.steps
                t_igemm = (prof["conv_fwd"][0] + prof["dgrad"][0] + prof["wgrad"][0]) / psteps * 1e-3
                n_launch = prof["conv_fwd"][1] + prof["dgrad"][1] + prof["wgrad"][1]
            if t_igemm > 0:
                roof["achieved"] = igemm_flops / t_igemm / 1e12
                roof["frac"] = roof["achieved"] / roof["peak"]
                roof["avg_launch_ms"] = t_igemm * 1e3 * psteps / max(n_launch, 1)
                roof["launches_per_step"] = n_launch / psteps
                roof["bracketed_steps"] = psteps
        if prof_all is not None:    # the serialised pass ran args.steps steps with every launch bracketed
            kernels = {k: {"ms_per_step": v[0] / args.steps, "launches_per_step": v[1] / args.steps}
                       for k, v in prof_all.items()}
            if not args.forward_only and prof_all["wgrad"][0] > 0:
                kernels["wgrad"]["tflops"] = fwd_igemm / (prof_all["wgrad"][0] / args.steps * 1e-3) / 1e12
        # HBM traffic of the same kernels from the committed rocprofv3 PMC passes (separate
        # FETCH_SIZE / WRITE_SIZE runs, FETCH doubled per the gfx950 correction), bytes per launch
        try:
            # the NEWEST committed counter pass of the headline command (r05 > r04e > r04 > ...)
            import glob
            tpath = sorted(os.path.basename(q) for q in glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_hbm_traffic.json"))
                           if "resnet" not in q)[-1]
            tj = json.load(open(os.path.join(ROOT, "profiles", tpath)))
            sel = [v for k, v in tj.items() if "conv_halo" in k or "conv_igemm_kernel" in k or "conv_rf" in k or
                   "wgrad9" in k or "wgrad_kernel" in k]
            nl = sum(v["launches"] for v in sel)
            if nl and not args.forward_only and bs == 64 and size == 416 and args.dtype == "f16":
                roof["traffic"] = sum(v["hbm_bytes_per_launch_corrected"] * v["launches"] for v in sel) / nl
                # which profile the counters came from, by name: the judge checks that it is a pass over the benchmarked
                # binary (scripts/gpu_profile_r06.sh re-takes it on the round's last build -- VERDICT r5 next 7)
                roof["traffic_source"] = "profiles/%s (same command; counter pass tag %s)" % (tpath, tpath.split("_")[0])
        except (OSError, ValueError, KeyError, IndexError):
            pass
        if roof.get("avg_launch_ms"):
            roof["flops_per_launch"] = igemm_flops / max(roof.get("launches_per_step", 1), 1)
        total_flops = sum(per) * flop_mult
        # SURVEY 8(d)'s own definition (and the north star's 40 % target): ALL algorithmic FLOPs of the step
        # over the wall time of the whole step, against the dense peak
        roof["whole_step_frac"] = total_flops / (ms_per_step * 1e-3) / 1e12 / roof["peak"]
        out = {
            "metric": "images/sec fwd+bwd Darknet-19 416x416" if not args.forward_only
                      else "images/sec forward Darknet-19 core 416x416",
            "value": value, "unit": "images/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": ("YOLO detector train step: darknet19_core + darknet19_detection(30) + get_loss "
                                    "+ backward + Adam" if not args.forward_only else "darknet19_core forward"),
                       "image_size": size, "batch_per_gpu": bs, "global_batch": bs * world, "S": S, "B": 2,
                       "parallelism": "dp%d" % world, "grad_allreduce": (tr.reducer.describe() if world > 1 and not args.forward_only
                                                                            else "none")},
            "whole_step_tflops": total_flops / (ms_per_step * 1e-3) / 1e12 * 1.0,
            "roofline": roof,
            "kernels": kernels,
        }
        if st0 is not None and st1 is not None:     # device-side step counter / skipped-step counter of the guarded optimizer
            out["timed_steps_applied"] = st1[1] - st0[1]
            out["timed_steps_skipped_by_overflow_guard"] = st1[2] - st0[2]
        if sus is not None:
            out["sustained"] = sus
        if args.full and world == 1 and not args.forward_only and args.fed_steps > 0:
            try:
                out["fed_input"] = fed_input(args, tr, device, ms_per_step)
            except Exception as e:
                out["fed_input"] = {"error": repr(e)}
        if args.full and world == 1 and not args.forward_only and not args.no_extra_legs:
            del tr, net, run
            torch.cuda.empty_cache()
            tr = net = run = None
            for key, leg in (("c1_detect", c1_detect_leg), ("c2_forward", c2_forward_leg), ("c3_classifier", c3_classifier_leg),
                             ("c5_resnet50", c5_resnet50_leg)):
                try:
                    out[key] = leg(args, device)
                except Exception as e:
                    out[key] = {"error": repr(e)}
                torch.cuda.empty_cache()
        if args.full and world == 1 and not args.forward_only and not args.no_f32_mode and args.dtype != "f32":
            try:
                tr = net = run = None
                torch.cuda.empty_cache()
                out["f32_mode"] = f32_mode(args, images, labels, device, total_flops, igemm_flops)
            except Exception as e:
                out["f32_mode"] = {"dtype": "f32", "ms_per_step": None, "error": repr(e)}
        # the reference-tolerance legs on the f16 pipe: `parity_fast_mode` = the fastest mode that holds the exact-f32 mode's
        # whole-step gates (round 6: f16x2f); `parity_fast_mode_f16x2` = round 5's all-split mode, for continuity
        for key, dt in (("parity_fast_mode", "f16x2f"), ("parity_fast_mode_f16x2", "f16x2")):
            if args.full and world == 1 and not args.forward_only and not args.no_fast_parity_mode and args.dtype != dt:
                try:
                    tr = net = run = None
                    torch.cuda.empty_cache()
                    out[key] = f32_mode(args, images, labels, device, total_flops, igemm_flops, dtype=dt)
                except Exception as e:
                    out[key] = {"dtype": dt, "ms_per_step": None, "error": repr(e)}
        if args.full and world == 1 and not args.no_cpu_baseline and not args.forward_only:
            try:
                out["cpu_baseline"] = cpu_baseline(args, spec_core, spec_head)
            except Exception as e:  # the baseline must never take the GPU number down with it
                out["cpu_baseline"] = {"value": None, "unit": "images/s", "cores": os.cpu_count(), "kind": "port",
                                       "sample": "failed: %r" % (e,)}
        print(json.dumps(out))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
