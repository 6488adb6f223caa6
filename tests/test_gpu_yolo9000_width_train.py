"""The wide trainer at YOLO9000's real width on the GPU: chain-wide.cfg with 28,269 filters over the 9,418-node tree
(tests/_yolo9000_cases.py write_yolo9000_width_files), batch 2 at 160 x 160 (M = 50, K = 128): one train step, the filter
gradient against float64 on the operands the device kept, within tests/test_gpu_wide_head_train.py's bound, and the update
moving W exactly where its gradient or the decay is nonzero."""
import numpy as np
import pytest

import _wide_head_cases as WH
import _yolo9000_cases as Y
from test_gpu_wide_head_train import SOLVER, _truths, dev, host
from tensorflow_yolo2_amd.utils import solver as S

pytestmark = pytest.mark.gpu


def test_one_step_at_28269_filters(tmp_path):
    import torch
    from tensorflow_yolo2_amd.yolo2_nets import net_utils, yolov2
    n, Kdim, Cout = 2, 128, WH.YOLO9000_FILTERS
    cfg = Y.write_yolo9000_width_files(tmp_path)
    sv = S.Solver(**dict(SOLVER, learning_rate=0.001))
    tr = yolov2.YOLOv2DarknetTrainer.from_cfg(cfg, batch=n, image_size=160, dtype="f16", wide_head=True, solver=sv, seed=3)
    assert (tr.wide.K, tr.wide.Cout) == (Kdim, Cout) and tr.tree.n == Y.NODES
    src = WH.random_weights_file(str(tmp_path / "wide.weights"), tr.cfg.file_layers, seed=Y.DETECTOR_WEIGHTS_SEED)
    net_utils.load_darknet_weights(tr, src)
    truth, ntruth = _truths(n)
    x = dev(np.random.default_rng(8).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8))
    W0 = host(tr.wide.W).reshape(Kdim, Cout)
    scale = tr.opts[0].scaler.scale
    loss = tr.step(x, truth=truth, ntruth=ntruth)
    torch.cuda.synchronize()
    assert np.isfinite(host(loss)).all() and tr.opts[0].scaler.state() == (0, 1, 0)
    xs, dy = host(tr.last_wide_x).reshape(-1, Kdim), host(tr.last_dnet).reshape(-1, Cout)
    M = xs.shape[0]
    assert M == n * 25
    xh = xs.astype(np.float16).astype(np.float64)
    dh = (np.float32(scale) * dy).astype(np.float32).astype(np.float16).astype(np.float64)
    assert np.isfinite(dh).all()
    ref = xh.T @ dh / scale
    bound = 2.0 * M * 2.0 ** -24 * (np.abs(xh).T @ np.abs(dh)) / scale + 1e-30
    dW = host(tr.wide.dW).reshape(Kdim, Cout)
    ratio = (np.abs(dW.astype(np.float64) - ref) / bound).max()
    print("trainer (%d, %d, %d) at loss scale %g: dW largest |got - ref| / bound = %.4f, nonzero dy columns %d" %
          (M, Kdim, Cout, scale, ratio, (dy != 0).any(0).sum()))
    assert ratio <= 1.0, ratio
    assert (dy != 0).any() and not (dy != 0).any(0).all()                 # the tree loss leaves most class columns zero
    # accum starts at zero: the step is the specification's, and W stays where neither dW nor the decay term is nonzero
    from test_solver_host import ulps
    W1 = host(tr.wide.W).reshape(Kdim, Cout)
    want, _acc = S.sgd_step(W0, np.zeros_like(W0), dW, S.current_rate(sv, 1), sv.momentum, sv.decay, True)
    assert ulps(W1, want).max() <= 1
    still = (dW == 0) & (np.float32(sv.decay) * W0 == 0)
    assert not (W1 != W0)[still].any() and (W1 != W0).any()
