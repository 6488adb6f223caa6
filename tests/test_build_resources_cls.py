"""CPU test of the BUILT augment.o (no GPU): the two instantiations of the classifier's warp kernel exist and neither
spills nor owns scratch, and the register count of the detector's augmentation kernel beside them is on record."""
import os

import pytest

from test_build_resources import LLVM, ROOT, kernel_metadata


def test_warp_kernels_are_built_without_spills_or_scratch():
    obj = os.path.join(ROOT, "tensorflow_yolo2_amd", "csrc", "augment.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("augment.o not built here (run __graft_entry__.build())")
    meta = kernel_metadata(obj)
    warp = sorted(m for m in meta if "warp_u8_kernel" in m[0])
    # warp_u8_kernel<false> (no parameter rows: identity maps, no colour stage) and warp_u8_kernel<true>
    assert len(warp) == 2 and "ILb0E" in warp[0][0] and "ILb1E" in warp[1][0], [m[0] for m in meta]
    for name, vgpr, spill, scratch in warp:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 128, (name, vgpr)                # four waves per SIMD and more, whatever LDS allows
    aug = sorted(m for m in meta if "augment_u8_kernel" in m[0])
    assert len(aug) == 2, [m[0] for m in meta]
    # augment_u8_kernel<1> / <4> beside them: spill-free as before; their VGPR counts ride in the message
    assert all(spill == 0 and scratch == 0 for _, _, spill, scratch in aug), \
        "augment_u8_kernel (name, VGPRs, spilled, scratch): %r" % (aug,)
    print("augment_u8_kernel VGPRs: %r; warp_u8_kernel VGPRs: %r" % ([(m[0], m[1]) for m in aug],
                                                                    [(m[0], m[1]) for m in warp]))
