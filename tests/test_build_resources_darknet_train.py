"""CPU test of the BUILT ext.o (no GPU): the two instantiations of the kernel of y2_passthrough_concat_darknet_backward
(16-byte and 4-byte slots) exist, spill nothing, own no scratch and stay at full occupancy (64 VGPRs: 8 waves per SIMD)."""
import os

import pytest

from test_build_resources import LLVM, ROOT, kernel_metadata


def test_darknet_route_backward_kernels_are_built_without_spills_or_scratch():
    obj = os.path.join(ROOT, "tensorflow_yolo2_amd", "csrc", "ext.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("ext.o not built here (run __graft_entry__.build())")
    meta = kernel_metadata(obj)
    back = sorted(m for m in meta if "darknet_route_backward_kernel" in m[0])
    # darknet_route_backward_kernel<1>, <4>
    assert len(back) == 2 and "ILi1E" in back[0][0] and "ILi4E" in back[1][0], [m[0] for m in meta]
    for name, vgpr, spill, scratch in back:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 64, (name, vgpr)
    # the counts tests/test_build_resources_darknet.py holds the forward kernels to are not disturbed by the name
    assert not any("passthrough_concat_darknet_kernel" in m[0] or "u8_bgr_to_f32_rgb_kernel" in m[0] for m in back)
    print("darknet route backward kernels (name, VGPRs, spilled, scratch): %r" % (back,))
