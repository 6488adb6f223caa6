"""Y2_FP8 (MXFP8 inference) without a GPU: the public constant, context planning of the three Darknet-19 specs, the
package's dtype switch, and the torch restatement of the quantiser (tests/_mx8.py) against hand-worked cases."""
import ctypes as C

import torch

from _mx8 import mx_dequantize_ref, mx_quantize_ref


def test_fp8_dtype_and_planning_without_gpu():
    from tensorflow_yolo2_amd import _lib
    from tensorflow_yolo2_amd.yolo2_nets import darknet
    assert _lib.DTYPES["fp8"] == 5 and _lib.DTYPES["mxfp8"] == 5 and _lib.Y2_FP8 == 5
    lib = _lib.load()
    for kind in (0, 1, 2):
        spec = _lib.darknet19_spec(kind, 30)
        flat = (C.c_int * (4 * len(spec)))(*[v for s in spec for v in s])
        tail = 1 if kind == 2 else 0
        sizes = {}
        for dtype in (1, 5):
            h = C.c_void_p()
            _lib.check(lib.y2_ctx_create(C.byref(h), flat, len(spec), 18, tail, 7, 2, 224, 224, dtype))
            sizes[dtype] = (lib.y2_param_count(h), lib.y2_workspace_bytes(h, 0))
            lib.y2_ctx_destroy(h)
        assert sizes[5][0] == sizes[1][0]
        # the e4m3 filters + scale planes and the e4m3 input scratch come on top of the f16 mode's tensors
        assert sizes[5][1] > sizes[1][1]
    # the op-level forward sizes its quantisation workspace
    assert lib.y2_conv2d_workspace_bytes(2, 13, 13, 64, 30, 3, 5) > 0
    assert lib.y2_ctx_create(C.byref(C.c_void_p()), flat, len(spec), 18, tail, 7, 2, 224, 224, 6) < 0
    darknet.set_default_dtype("fp8")
    darknet.set_default_dtype("f16")


def _block(vals):
    x = torch.zeros(32, dtype=torch.float32)
    x[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
    return x


def _q(x):
    q, s = mx_quantize_ref(x.reshape(1, -1))
    return q.reshape(-1), int(s.reshape(-1)[0]) - 127


def test_quantiser_restatement_hand_cases():
    # m = 0.875 exactly: amax = 0.875 * 2^E = 448 * 2^(E - 9) -> e = E - 9 and the element is 448 (0x7E)
    q, e = _q(_block([0.875 * 2.0 ** 3]))
    assert e == 3 - 9 and int(q[0]) == 0x7E
    # one ulp above: m > 0.875 -> e = E - 8; 7.0000005 / 2^-5 = 224.00002 -> 224 = 1.75 * 2^7 (0x76)
    q, e = _q(_block([float(torch.nextafter(torch.tensor(7.0), torch.tensor(8.0)))]))
    assert e == 3 - 8 and int(q[0]) == 0x76
    # amax = 448 * 2^e exactly for e = 2: 1792 -> scale 2^2, element 448
    q, e = _q(_block([1792.0, 1.0]))
    assert e == 2 and int(q[0]) == 0x7E and int(q[1]) == 0x28      # 1 / 4 = 2^-2: exponent field 5, mantissa 0
    # ... one ulp above 1792: the next scale, 1792.0001 / 8 = 224.00002 -> 224
    q, e = _q(_block([float(torch.nextafter(torch.tensor(1792.0), torch.tensor(2048.0)))]))
    assert e == 3 and int(q[0]) == 0x76
    # all-zero block: the smallest scale (byte 0), zero elements
    q, e = _q(_block([]))
    assert e == -127 and int(q.abs().sum()) == 0
    # negative values: sign bit, same magnitude code; -448 * 2^-4 -> e = -4
    q, e = _q(_block([-28.0, 28.0, -3.5]))
    assert e == -4 and int(q[0]) == 0xFE and int(q[1]) == 0x7E and int(q[2]) == 0x80 | 0x66   # 3.5 * 16 = 56 = 1.75 * 2^5
    # subnormals of e4m3 (quantum 2^-9 of the scaled value): amax 448 keeps e = 0; 3 * 2^-9 -> code 3, 2^-10 -> 0 (tie to
    # even), 3 * 2^-10 -> 2 (tie to even), 2^-6 * 15 / 16 -> 8 (rounds up into the smallest normal)
    q, e = _q(_block([448.0, 3 * 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -6 * 15 / 16]))
    assert e == 0 and [int(v) for v in q[:5]] == [0x7E, 3, 0, 2, 8]
    # the round trip reproduces values already on the grid
    x = _block([448.0, -3 * 2.0 ** -9, 1.5, -240.0])
    qq, ss = mx_quantize_ref(x.reshape(1, -1))
    assert torch.equal(mx_dequantize_ref(qq, ss).reshape(-1), x.to(torch.float64))
