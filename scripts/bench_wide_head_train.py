"""What training YOLO9000's last layer costs: K = 1024, Cout = 28,269, one 544 x 544 image (M = 289 cells) and a batch of
32 (M = 9,248).  Per shape, (a) against (b):

  data gradient    (a) y2_wide_head_backward_input: fp32 dy converted in the kernel, packed f16 filters, the plan's split
                       and its finish pass, fp32 dx
                   (b) torch.matmul(dy16, W16.T).float() on f16 copies of the same operands (the copies are not timed)
  filter gradient  (a) y2_wide_head_backward_filter: fp32 x and dy converted in the kernel, fp32 dW, and its db launch
                   (b) torch.matmul(x16.T, dy16).float() and dy.sum(0): the vendor GEMM, this project's GEMM ceiling
  update           (a) y2_wide_head_sgd_step: W, accum, dW read, W, accum and both f16 images written
                   (b) those bytes at the 5 TB/s the streaming kernels of this library reach

The expectation written down before measuring is in DESIGN.md, "Training the wide head".  An expectation, not a gate.
Then the step of the chain-wide model at the real width (tests/_yolo9000_cases.py: 28,269 filters, 9,418 nodes; batch 2
at 160 x 160, M = 50, K = 128) next to the same trainer's forward pass, and the largest |got - ref| / bound of the product
parity at the shapes of tests/test_gpu_wide_head_train.py.

HIP events around blocks of --inner calls; the legs alternate inside every repetition and the median over --reps
repetitions is reported.

    python scripts/bench_wide_head_train.py --out profiles/wide_head_train.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_TBS = 5.0                    # what the streaming kernels of this library reach


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--cout", type=int, default=28269)
    ap.add_argument("--cells", type=int, default=289)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="skip the chain-wide trainer's step")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    from tensorflow_yolo2_amd import engine as E
    from tensorflow_yolo2_amd.utils import solver as S
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
        return {k: statistics.median(v) for k, v in us.items()}

    Kd, Cout = args.k, args.cout
    rng = np.random.default_rng(0)
    Wt = rng.standard_normal((Kd, Cout), np.float32) * np.float32(0.05)
    wide = E.WideHead(Kd, Cout)
    wide.load(Wt, np.zeros(Cout, np.float32))
    W16 = torch.from_numpy(Wt).cuda().half()
    opt = E.WideHeadSGD(wide, S.Solver(learning_rate=1e-6, policy="constant", burn_in=0, steps=(), scales=()))
    lib = wide.lib
    say("Training the wide head, K = %d, Cout = %d; HIP events, median of %d alternating blocks of %d calls, microseconds "
        "per call" % (Kd, Cout, args.reps, args.inner))
    say("    M  GFLOP  splits dx dW  (a) dx  (b) matmul + float  (a)/(b)  (a) dW + db  (b) matmul + float + sum  (a)/(b)")
    for batch in [int(v) for v in args.batches.split(",")]:
        M = batch * args.cells
        x = torch.from_numpy(rng.standard_normal((M, Kd), np.float32)).cuda()
        dy = torch.from_numpy(rng.standard_normal((M, Cout), np.float32) * np.float32(0.05)).cuda()
        x16, dy16 = x.half(), dy.half()
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        props = torch.cuda.get_device_properties(0)
        assert lib.y2_wide_head_train_plan(M, Kd, Cout, props.multi_processor_count, ctypes.byref(a), ctypes.byref(b)) == 0
        keep = {}
        wide.backward(x, dy, 1.0)               # allocates dW, db, dx and the workspace outside the timing
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        ws, dx = wide._ws, wide._dx[M]
        nws = ws.numel() if ws is not None else 0

        def a_dx():
            E.check(lib.y2_wide_head_backward_input(p(dy), p(wide.packed2), M, Kd, Cout, 1.0, p(dx), p(ws), nws, 0, None))

        def b_dx():
            keep["dx"] = torch.matmul(dy16, W16.t()).float()

        def a_dw():
            E.check(lib.y2_wide_head_backward_filter(p(x), p(dy), M, Kd, Cout, 1.0, p(wide.dW), p(wide.db), p(ws), nws, 0,
                                                     None))

        def b_dw():
            keep["dW"] = torch.matmul(x16.t(), dy16).float()
            keep["db"] = dy.sum(0)

        med = medians([("a_dx", a_dx), ("b_dx", b_dx), ("a_dw", a_dw), ("b_dw", b_dw)])
        say("%5d  %5.1f  %6d %5d  %6.1f  %18.1f  %7.2f  %11.1f  %24.1f  %7.2f"
            % (M, 2.0 * M * Kd * Cout / 1e9, a.value, b.value, med["a_dx"], med["b_dx"], med["a_dx"] / med["b_dx"],
               med["a_dw"], med["b_dw"], med["a_dw"] / med["b_dw"]))
        del keep, x16, dy16, x, dy
    mb = (5 * Kd * Cout * 4 + wide.packed.numel() + wide.packed2.numel()) / 1e6
    med = medians([("step", lambda: opt.step(1.0))])
    say()
    say("Update (W, accum, dW read; W, accum, both images written): %.1f MB, %.1f us at %.0f TB/s; (a) y2_wide_head_sgd_step "
        "%.1f us = %.2f TB/s, (a)/(b) %.2f" % (mb, mb / STREAM_TBS, STREAM_TBS, med["step"], mb / med["step"],
                                               med["step"] / (mb / STREAM_TBS)))
    del wide, opt, W16
    torch.cuda.empty_cache()

    if not args.no_model:
        import _wide_head_cases as WH
        import _yolo9000_cases as Y
        from tensorflow_yolo2_amd.yolo2_nets import yolov2
        with tempfile.TemporaryDirectory() as tmp:
            cfg = Y.write_yolo9000_width_files(tmp)
            sv = S.Solver(learning_rate=1e-4, policy="constant", burn_in=0, steps=(), scales=())
            tr = yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, batch=2, image_size=160, dtype="f16", wide_head=True, solver=sv)
        images = torch.from_numpy(rng.integers(0, 256, (2, 160, 160, 3), dtype=np.uint8)).cuda()
        truth = np.zeros((2, 30, 5), np.float32)
        truth[0, 0], truth[0, 1] = (41.6, 51.2, 45.0, 58.0, 90), (54.4, 44.8, 40.0, 36.0, 125)
        truth, ntruth = torch.from_numpy(truth).cuda(), torch.from_numpy(np.array([2, 0], np.int32)).cuda()
        med = medians([("forward", lambda: tr.forward(images, True)), ("step", lambda: tr.step(images, truth=truth, ntruth=ntruth))])
        say()
        say("chain-wide at the real width (28,269 filters over 9,418 nodes; batch 2 at 160 x 160, M = 50, K = 128, the host's "
            "launches included): forward(training) %.1f us, step %.1f us" % (med["forward"], med["step"]))
        del tr

    if not args.no_parity:
        import test_gpu_wide_head_train as T
        say()
        say("Product parity against numpy float64 on the operands as the kernels round them, every split of the plan: the "
            "lines of tests/test_gpu_wide_head_train.py (its gate is 1)")
        import contextlib
        import io
        for shape in T.SHAPES:
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                T.check_products(*shape)
            say(buf.getvalue().strip())
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
