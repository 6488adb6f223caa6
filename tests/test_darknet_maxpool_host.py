"""utils/darknet_maxpool.py, the specification of Darknet's `[maxpool] size=2 stride=1`, against an independent
restatement (pad bottom and right with -inf, the maximum of the four shifts), torch float64 autograd of that restatement,
and hand-built cases for the tie rule and the order of the four-window sum."""
import numpy as np
import pytest
import torch

from tensorflow_yolo2_amd.utils.darknet_maxpool import FLT_MAX, maxpool_s1, maxpool_s1_backward

SHAPES = [(1, 1, 1, 1), (1, 1, 2, 4), (1, 2, 1, 3), (2, 3, 5, 12), (1, 13, 13, 8), (2, 6, 4, 5)]


def _restated(x):
    """x torch [N,H,W,C] -> the same pool through padding and shifts"""
    n, h, w, c = x.shape
    p = torch.full((n, h + 1, w + 1, c), -float("inf"), dtype=x.dtype)
    p = torch.cat([torch.cat([x, p[:, :h, w:]], dim=2), p[:, h:]], dim=1)
    return torch.maximum(torch.maximum(p[:, :h, :w], p[:, :h, 1:]), torch.maximum(p[:, 1:, :w], p[:, 1:, 1:]))


@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_the_restatement(shape):
    rng = np.random.default_rng(sum(shape))
    x = rng.standard_normal(shape).astype(np.float32)
    assert np.array_equal(maxpool_s1(x), _restated(torch.as_tensor(x)).numpy())
    ties = rng.integers(-2, 3, shape).astype(np.float32)
    assert np.array_equal(maxpool_s1(ties), _restated(torch.as_tensor(ties)).numpy())


@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_float64_autograd_on_tie_free_input(shape):
    rng = np.random.default_rng(7 + sum(shape))
    x = rng.permutation(int(np.prod(shape))).reshape(shape).astype(np.float32)     # all distinct: no ties
    dy = rng.standard_normal(shape).astype(np.float32)
    xt = torch.as_tensor(x, dtype=torch.float64).requires_grad_(True)
    _restated(xt).backward(torch.as_tensor(dy, dtype=torch.float64))
    ref = xt.grad.numpy()
    got = maxpool_s1_backward(x, dy)
    assert got.dtype == np.float32
    # up to four float32 addends: three roundings of at most 2^-24 each, relative to the sum of magnitudes
    bound = 3 * 2.0 ** -24 * 4 * np.abs(dy).max()
    assert np.abs(got - ref).max() <= bound


def test_constant_map_routes_every_gradient_to_the_first_tap():
    rng = np.random.default_rng(3)
    x = np.full((2, 4, 5, 3), 1.5, np.float32)
    dy = rng.standard_normal(x.shape).astype(np.float32)
    dx = maxpool_s1_backward(x, dy)
    assert np.array_equal(dx.view(np.uint32), (dy + np.float32(0)).view(np.uint32))


def test_one_by_one_map_is_the_identity():
    x = np.array([-3.25, 0.0, 7.0], np.float32).reshape(1, 1, 1, 3)
    dy = np.array([1.0, -2.0, 0.5], np.float32).reshape(1, 1, 1, 3)
    assert np.array_equal(maxpool_s1(x), x)
    assert np.array_equal(maxpool_s1_backward(x, dy), dy)


def test_four_window_sum_runs_in_ascending_anchor_order():
    """the centre of a 3x3 map wins the four windows that hold it; with dy = (2^24, 1, -2^24, 1) at the anchors (0,0), (0,1),
    (1,0), (1,1) the float32 sum is ((2^24 + 1) - 2^24) + 1 = 1 in that order and 2 in any order that adds the ones last"""
    x = np.zeros((1, 3, 3, 1), np.float32)
    x[0, 1, 1, 0] = 9.0
    dy = np.zeros((1, 3, 3, 1), np.float32)
    dy[0, 0, 0, 0], dy[0, 0, 1, 0], dy[0, 1, 0, 0], dy[0, 1, 1, 0] = 2.0 ** 24, 1.0, -2.0 ** 24, 1.0
    dy[0, 2, 2, 0] = 5.0                                       # window (2,2) holds x(2,2) alone
    dx = maxpool_s1_backward(x, dy)
    assert dx[0, 1, 1, 0] == 1.0
    want = np.zeros((1, 3, 3, 1), np.float32)
    want[0, 1, 1, 0], want[0, 2, 2, 0] = 1.0, 5.0
    # the other windows: (0,2) -> x(0,2) first, (1,2) -> x(1,2), (2,0) -> x(2,0), (2,1) -> x(2,1): their dy is 0
    assert np.array_equal(dx, want)


def test_signed_zeros_and_nans():
    nan = np.float32("nan")
    # one row, C = 1: windows (0,0..3) over [-0, +0, nan, nan]
    x = np.array([-0.0, 0.0, nan, nan], np.float32).reshape(1, 1, 4, 1)
    y = maxpool_s1(x)
    # window 0: -0 first, +0 is not greater: -0 stays.  window 1: +0, nan never chosen.  windows 2 and 3: NaNs alone
    want = np.array([-0.0, 0.0, -FLT_MAX, -FLT_MAX], np.float32).reshape(1, 1, 4, 1)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    dy = np.array([1.0, 2.0, 4.0, 8.0], np.float32).reshape(1, 1, 4, 1)
    dx = maxpool_s1_backward(x, dy)
    assert np.array_equal(dx, np.array([1.0, 2.0, 0.0, 0.0], np.float32).reshape(1, 1, 4, 1))


def test_refuses_what_is_no_float32_map():
    with pytest.raises(ValueError):
        maxpool_s1(np.zeros((2, 3, 4), np.float32))
    with pytest.raises(ValueError):
        maxpool_s1(np.zeros((1, 2, 2, 1), np.float64))
    with pytest.raises(ValueError):
        maxpool_s1_backward(np.zeros((1, 2, 2, 1), np.float32), np.zeros((1, 2, 2, 2), np.float32))
