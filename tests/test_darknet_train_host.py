"""CPU tests of what the "darknet"-topology trainer adds on the host: the gradient of Darknet's reorg as the inverse of
the index table (utils/darknet_reorg.py), against the forward function and against torch autograd's vector-Jacobian
product of the gather in float64, and the train caller's new arguments."""
import numpy as np
import pytest

from tensorflow_yolo2_amd.utils import darknet_reorg as RG

SHAPES = [(1, 2, 2, 4), (2, 4, 6, 8), (1, 6, 4, 8), (2, 6, 6, 64)]        # (N, H, W, C) of the fine map


@pytest.mark.parametrize("shape", SHAPES)
def test_reorg_backward_is_the_inverse_permutation(shape):
    n, h, w, c = shape
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    y = RG.reorg_darknet(x)
    assert y.shape == (n, h // 2, w // 2, 4 * c)
    back = RG.reorg_darknet_backward(y)
    assert back.shape == x.shape and back.dtype == x.dtype
    np.testing.assert_array_equal(back, x)
    d = rng.standard_normal(y.shape).astype(np.float32)
    np.testing.assert_array_equal(RG.reorg_darknet(RG.reorg_darknet_backward(d)), d)


@pytest.mark.parametrize("shape", SHAPES)
def test_reorg_backward_is_autograd_vjp_of_the_gather(shape):
    import torch
    n, h, w, c = shape
    rng = np.random.default_rng(7 + sum(shape))
    x = torch.tensor(rng.standard_normal(shape), dtype=torch.float64, requires_grad=True)
    js, is_, cs = (torch.as_tensor(t) for t in RG.reorg_darknet_table(h, w, c))
    y = x[:, js, is_, cs]
    dout = rng.standard_normal(tuple(y.shape))
    y.backward(torch.as_tensor(dout))
    np.testing.assert_array_equal(RG.reorg_darknet_backward(dout), x.grad.numpy())


def test_passthrough_backward_splits_at_four_cf():
    rng = np.random.default_rng(11)
    n, h, w, cf, cc = 2, 3, 2, 8, 5
    fine = rng.standard_normal((n, 2 * h, 2 * w, cf)).astype(np.float32)
    coarse = rng.standard_normal((n, h, w, cc)).astype(np.float32)
    dfine, dcoarse = RG.passthrough_concat_darknet_backward(RG.passthrough_concat_darknet(fine, coarse), cf)
    np.testing.assert_array_equal(dfine, fine)
    np.testing.assert_array_equal(dcoarse, coarse)
    dout = rng.standard_normal((n, h, w, 4 * cf + cc)).astype(np.float32)
    dfine, dcoarse = RG.passthrough_concat_darknet_backward(dout, cf)
    np.testing.assert_array_equal(dcoarse, dout[..., 4 * cf:])
    np.testing.assert_array_equal(dfine, RG.reorg_darknet_backward(dout[..., :4 * cf]))
    with pytest.raises(ValueError):
        RG.passthrough_concat_darknet_backward(dout, 6)
    with pytest.raises(ValueError):
        RG.passthrough_concat_darknet_backward(dout[..., :4 * cf], cf)


def test_train_caller_arguments():
    from tensorflow_yolo2_amd.pascal import pascal_train_yolov2 as T
    base = ["--devkit", "kit"]
    a = T.parse_args(base)
    assert a.topology == "paper" and a.darknet_weights is None
    a = T.parse_args(base + ["--darknet-weights", "m.weights"])
    assert a.topology == "darknet" and a.darknet_weights == "m.weights"
    assert T.parse_args(base + ["--darknet-weights", "m.weights", "--topology", "darknet"]).topology == "darknet"
    a = T.parse_args(base + ["--topology", "darknet", "--darknet-backbone", "core.conv.23"])
    assert a.topology == "darknet" and a.darknet_backbone == "core.conv.23"
    assert T.parse_args(base + ["--darknet-backbone", "core.conv.23"]).topology == "paper"
    for bad in (["--darknet-weights", "m.weights", "--darknet-backbone", "core.conv.23"],
                ["--darknet-weights", "m.weights", "--imagenet-ckpt-dir", "d"],
                ["--darknet-weights", "m.weights", "--topology", "paper"]):
        with pytest.raises(SystemExit):
            T.parse_args(base + bad)
