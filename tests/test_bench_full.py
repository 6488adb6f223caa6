"""`bench.py` runs lean by default: a plain run sets up, warms up, times its --steps steps and prints the one JSON line;
every leg that takes steps of its own (serialised per-class pass, sustained region, fed input, the other configurations,
f32 / parity modes, CPU baseline) runs under `--full` only.  The option parsing is checked without a GPU, the step
counts of both forms on one (-m gpu) inside this process, at batch 8."""
import json
import sys

import pytest

import bench

MOVED = ("sustained", "fed_input", "c1_detect", "c2_forward", "c3_classifier", "c5_resnet50", "f32_mode",
         "parity_fast_mode", "parity_fast_mode_f16x2", "cpu_baseline")


def _main(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.main()


def test_full_is_an_option_and_off_by_default(monkeypatch, capsys):
    with pytest.raises(SystemExit) as e:
        _main(monkeypatch, "--help")
    assert e.value.code == 0
    assert "--full" in capsys.readouterr().out


def test_separate_kernel_pass_needs_full(monkeypatch, capsys):
    """--kernel-events separate has nothing but the pass of its own to measure in: an error without --full, not a
    silent line without a roofline"""
    with pytest.raises(SystemExit) as e:
        _main(monkeypatch, "--kernel-events", "separate")
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err


def _counted_run(monkeypatch, capsys, *argv):
    """bench.main() in this process; (the line it returned, the one JSON line it printed, DetectorTrainer.step calls)"""
    from tensorflow_yolo2_amd.trainer import DetectorTrainer
    calls = [0]
    step = DetectorTrainer.step

    def counting(self, *a, **k):
        calls[0] += 1
        return step(self, *a, **k)
    monkeypatch.setattr(DetectorTrainer, "step", counting)
    out = _main(monkeypatch, "--gpus", "1", "--batch", "8", *argv)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return out, json.loads(lines[0]), calls[0]


@pytest.mark.gpu
def test_plain_run_does_the_timed_steps_only(monkeypatch, capsys):
    out, line, calls = _counted_run(monkeypatch, capsys, "--steps", "3", "--warmup", "2")
    assert calls == 2 + 3                               # warm-up + timed steps, nothing after them
    assert line["metric"] == "images/sec fwd+bwd Darknet-19 416x416" and line["unit"] == "images/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f16"
    assert line["steps"] == 3 and line["warmup"] == 2
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    # the event brackets are part of the timed steps: their roofline stays in the plain line
    assert line["roofline"]["frac"] > 0 and line["roofline"]["bracketed_steps"] == 1
    assert line["timed_steps_applied"] + line["timed_steps_skipped_by_overflow_guard"] == 3
    assert line["kernels"] is None
    assert not [k for k in MOVED if k in line]
    assert out["value"] == line["value"]


@pytest.mark.gpu
def test_full_run_adds_the_legs_it_is_asked_for(monkeypatch, capsys):
    """--full with the long legs switched off by their own options: the serialised pass (--steps more steps), the
    sustained region and the fed loop (3 warm-up steps of its own) run after the timed steps"""
    out, line, calls = _counted_run(monkeypatch, capsys, "--steps", "3", "--warmup", "2", "--full", "--sustain-steps", "4",
                                    "--fed-steps", "2", "--no-extra-legs", "--no-f32-mode", "--no-fast-parity-mode",
                                    "--no-cpu-baseline")
    assert calls == (2 + 3) + 3 + 4 + (3 + 2)
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    assert abs(line["value"] - 8 / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert line["roofline"]["frac"] > 0
    for k in ("conv_fwd", "dgrad", "wgrad"):
        assert line["kernels"][k]["ms_per_step"] > 0 and line["kernels"][k]["launches_per_step"] > 0
    assert line["sustained"]["steps"] == 4 and line["sustained"]["ms_per_step"] > 0
    assert line["fed_input"].get("error") is None and line["fed_input"]["steps"] == 2
    assert not [k for k in MOVED if k in line and k not in ("sustained", "fed_input")]
