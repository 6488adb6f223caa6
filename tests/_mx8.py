"""Torch restatement of the MXFP8 number format of Y2_FP8 (include/yolo2_hip.h): e4m3fn elements, one E8M0 scale per
32 consecutive values of the last axis.  Scale: the smallest e with amax <= 448 * 2^e -- frexp(amax) = m * 2^E,
e = E - 9 if m <= 0.875 else E - 8 -- clamped to [-127, 127], -127 for an all-zero block; elements RNE_e4m3(v / 2^e)
behind a +-448 clamp.  Test infrastructure only (CPU)."""
import numpy as np
import torch


def mx_quantize_ref(x):
    """x [..., C] (C % 32 == 0) -> (elements as uint8 [..., C], scale bytes uint8 [..., C / 32])"""
    x = torch.as_tensor(np.asarray(x, np.float32) if not torch.is_tensor(x) else x, dtype=torch.float32).cpu()
    shp = x.shape
    b = x.reshape(-1, shp[-1] // 32, 32)
    amax = b.abs().amax(-1)
    m, E = torch.frexp(amax)
    e = torch.where(m <= 0.875, E - 9, E - 8)
    e = torch.where(amax > 0, e, torch.full_like(e, -127)).clamp(-127, 127)
    v = torch.ldexp(b, (-e).to(torch.float32)[..., None])
    q = v.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return q.reshape(shp), (e + 127).to(torch.uint8).reshape(shp[:-1] + (shp[-1] // 32,))


def mx_dequantize_ref(q, s):
    """(elements, scale bytes) -> float64 values"""
    q = torch.as_tensor(q).cpu()
    s = torch.as_tensor(s).cpu()
    shp = q.shape
    v = q.reshape(-1, shp[-1] // 32, 32).view(torch.float8_e4m3fn).to(torch.float64)
    return (v * torch.pow(2.0, s.reshape(-1, shp[-1] // 32, 1).to(torch.float64) - 127.0)).reshape(shp)


def mx_round(x):
    """x [..., C] -> float64 values after one quantise / dequantise round trip"""
    return mx_dequantize_ref(*mx_quantize_ref(x))


def mx_round_filter(w):
    """HWIO filter [k, k, Cin, Cout] -> the same after the round trip over blocks of 32 input channels"""
    w = torch.as_tensor(np.asarray(w, np.float32))
    t = w.permute(0, 1, 3, 2).contiguous()            # [k, k, Cout, Cin]: a block = 32 input channels of one tap and cout
    return mx_round(t).permute(0, 1, 3, 2).contiguous()
