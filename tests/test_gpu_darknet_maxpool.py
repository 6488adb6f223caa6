"""y2_maxpool2x2s1 and y2_maxpool2x2s1_backward, Darknet's `[maxpool] size=2 stride=1`, against their numpy
specification (utils/darknet_maxpool.py) bit for bit: random inputs, inputs full of ties, signed zeros and NaN taps, the
16-byte and the one-float instantiations (C % 4, an unaligned pointer), more than one workgroup, outputs pre-filled with
NaN so that an element left unwritten shows; the backward pass twice for equal bits; and the refusals."""
import ctypes as C

import numpy as np
import pytest

from tensorflow_yolo2_amd.utils import darknet_maxpool as MP

pytestmark = pytest.mark.gpu

Y2_OK, Y2_ERR_ARG = 0, -1          # include/yolo2_hip.h
SHAPES = [(1, 1, 1, 1), (1, 1, 2, 4), (1, 2, 1, 3), (2, 3, 5, 12), (2, 13, 13, 512), (1, 19, 19, 64)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_raw(x, dy, offset=0):
    """both entry points on device copies of x and dy that start `offset` floats into their allocations, outputs filled
    with NaN beforehand -> (y, dx) as numpy"""
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    n, h, w, c = x.shape
    place = lambda a: torch.cat([torch.zeros(offset), torch.as_tensor(a).reshape(-1)]).cuda()[offset:]
    xd, dyd = place(x), place(dy)
    yd, dxd = place(np.full(x.shape, np.nan, np.float32)), place(np.full(x.shape, np.nan, np.float32))
    assert xd.data_ptr() % 16 == (4 * offset) % 16
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.y2_maxpool2x2s1(p(xd), p(yd), n, h, w, c, stream) == Y2_OK
    assert lib.y2_maxpool2x2s1_backward(p(xd), p(dyd), p(dxd), n, h, w, c, stream) == Y2_OK
    torch.cuda.synchronize()
    return yd.cpu().numpy().reshape(x.shape), dxd.cpu().numpy().reshape(x.shape)


def assert_is_specification(x, dy, offset=0):
    y, dx = run_raw(x, dy, offset)
    np.testing.assert_array_equal(bits(y), bits(MP.maxpool_s1(x)))
    np.testing.assert_array_equal(bits(dx), bits(MP.maxpool_s1_backward(x, dy)))


@pytest.mark.parametrize("shape", SHAPES)
def test_random_input_is_the_specification(shape):
    rng = np.random.default_rng(sum(shape))
    assert_is_specification(rng.standard_normal(shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32))


@pytest.mark.parametrize("shape", SHAPES)
def test_ties_are_the_specification(shape):
    rng = np.random.default_rng(11 + sum(shape))
    assert_is_specification(rng.integers(-2, 3, shape).astype(np.float32), rng.standard_normal(shape).astype(np.float32))


def test_unaligned_pointer_takes_the_scalar_path():
    rng = np.random.default_rng(5)
    shape = (2, 3, 5, 4)
    x = rng.integers(-2, 3, shape).astype(np.float32)
    assert_is_specification(x, rng.standard_normal(shape).astype(np.float32), offset=1)


@pytest.mark.parametrize("shape", [(1, 2, 1, 3), (2, 5, 7, 8), (1, 13, 13, 64)])
def test_signed_zeros_and_nans_are_the_specification(shape):
    rng = np.random.default_rng(23 + sum(shape))
    values = np.array([-0.0, 0.0, np.nan, np.nan, -1.0, 1.0], np.float32)
    x = values[rng.integers(0, len(values), shape)]
    dy = rng.standard_normal(shape).astype(np.float32)
    dy[rng.random(shape) < 0.2] = -0.0
    assert np.isnan(x).any() and (bits(x) == 0x80000000).any()
    assert_is_specification(x, dy)
    assert_is_specification(np.full(shape, np.nan, np.float32), dy)          # NaNs alone: -FLT_MAX, no gradient


def test_engine_wrappers_and_two_backward_runs():
    import torch
    from tensorflow_yolo2_amd import engine as E
    rng = np.random.default_rng(1)
    shape = (2, 13, 13, 512)
    x = rng.integers(-2, 3, shape).astype(np.float32)
    dy = rng.standard_normal(shape).astype(np.float32)
    xd, dyd = torch.as_tensor(x).cuda(), torch.as_tensor(dy).cuda()
    y = E.max_pool_2x2_s1(xd)
    first = E.max_pool_2x2_s1_backward(xd, dyd)
    second = E.max_pool_2x2_s1_backward(xd, dyd)
    assert tuple(y.shape) == shape and tuple(first.shape) == shape
    np.testing.assert_array_equal(bits(y.cpu().numpy()), bits(MP.maxpool_s1(x)))
    np.testing.assert_array_equal(bits(first.cpu().numpy()), bits(MP.maxpool_s1_backward(x, dy)))
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    with pytest.raises(ValueError):
        E.max_pool_2x2_s1(xd[0])
    with pytest.raises(ValueError):
        E.max_pool_2x2_s1_backward(xd, dyd[:1])
    with pytest.raises(ValueError):
        E.max_pool_2x2_s1(xd[:0])


def test_refuses_bad_arguments():
    import torch
    from tensorflow_yolo2_amd import _lib
    lib = _lib.load()
    x, dy, out = (torch.zeros(2 * 3 * 4, device="cuda") for _ in range(3))
    p = lambda t: C.c_void_p(t.data_ptr())
    null = C.c_void_p(0)
    fwd = lambda a, b, *dims: lib.y2_maxpool2x2s1(a, b, *dims, null)
    bwd = lambda a, b, c, *dims: lib.y2_maxpool2x2s1_backward(a, b, c, *dims, null)
    assert fwd(p(x), p(out), 1, 2, 3, 4) == Y2_OK
    assert bwd(p(x), p(dy), p(out), 1, 2, 3, 4) == Y2_OK
    bad_dims = ((0, 2, 3, 4), (1, 0, 3, 4), (1, 2, -1, 4), (1, 2, 3, 0), (1 << 15, 1 << 8, 1 << 8, 1), (2, 1 << 15, 1 << 15, 1),
                (1, 1, 1 << 16, 1 << 15))
    for args in [(null, p(out), 1, 2, 3, 4), (p(x), null, 1, 2, 3, 4)] + [(p(x), p(out)) + d for d in bad_dims]:
        assert fwd(*args) == Y2_ERR_ARG, args[2:]
        assert lib.y2_last_error().startswith(b"y2_maxpool2x2s1:")
    for args in [(null, p(dy), p(out), 1, 2, 3, 4), (p(x), null, p(out), 1, 2, 3, 4), (p(x), p(dy), null, 1, 2, 3, 4)] + \
            [(p(x), p(dy), p(out)) + d for d in bad_dims]:
        assert bwd(*args) == Y2_ERR_ARG, args[3:]
        assert lib.y2_last_error().startswith(b"y2_maxpool2x2s1_backward:")
    torch.cuda.synchronize()
