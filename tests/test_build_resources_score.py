"""CPU test of the BUILT score.o (no GPU): the scoring kernel of y2_score_views exists in its two forms (the logits staged
in LDS, and re-read from L2 where they do not fit), neither spills nor owns scratch, and both stay within 128 VGPRs."""
import os

import pytest

from test_build_resources import LLVM, ROOT, kernel_metadata


def test_score_kernels_are_built_without_spills_or_scratch():
    obj = os.path.join(ROOT, "tensorflow_yolo2_amd", "csrc", "score.o")
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("score.o not built here (run __graft_entry__.build())")
    meta = kernel_metadata(obj)
    score = sorted(m for m in meta if "score_views_kernel" in m[0])
    # score_views_kernel<false> (re-read) and score_views_kernel<true> (staged)
    assert len(score) == 2 and "ILb0E" in score[0][0] and "ILb1E" in score[1][0], [m[0] for m in meta]
    for name, vgpr, spill, scratch in score:
        assert spill == 0 and scratch == 0, (name, vgpr, spill, scratch)
        assert vgpr <= 128, (name, vgpr)                # four waves per SIMD and more
    print("score_views_kernel (name, VGPRs, spilled, scratch): %r" % (score,))
