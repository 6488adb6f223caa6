"""CPU test of the BUILT ext.o (no GPU): the kernels of y2_passthrough_concat_darknet (16-byte and 4-byte slots) and of
y2_u8_bgr_to_f32_rgb (four pixels per lane, and the tail) exist, spill nothing, own no scratch and stay at full
occupancy (64 VGPRs: 8 waves per SIMD)."""
import os

import pytest

from test_build_resources import LLVM, ROOT, kernel_metadata


def test_darknet_kernels_are_built_without_spills_or_scratch():
    obj = os.path.join(ROOT, "tensorflow_yolo2_amd", "csrc", "ext.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("ext.o not built here (run __graft_entry__.build())")
    meta = kernel_metadata(obj)
    concat = sorted(m for m in meta if "passthrough_concat_darknet_kernel" in m[0])
    convert = sorted(m for m in meta if "u8_bgr_to_f32_rgb_kernel" in m[0])
    # passthrough_concat_darknet_kernel<1>, <4>; u8_bgr_to_f32_rgb_kernel<false>, <true>
    assert len(concat) == 2 and "ILi1E" in concat[0][0] and "ILi4E" in concat[1][0], [m[0] for m in meta]
    assert len(convert) == 2 and "ILb0E" in convert[0][0] and "ILb1E" in convert[1][0], [m[0] for m in meta]
    for name, vgpr, spill, scratch in concat + convert:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 64, (name, vgpr)
    print("darknet kernels (name, VGPRs, spilled, scratch): %r" % (concat + convert,))
