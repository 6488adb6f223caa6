"""CPU test of the BUILT wide_head.o (no GPU), resource metadata only: the forward kernel exists once, spills nothing and
owns no scratch; its LDS is the two 64 KiB stages of the 256 x 256 x 64 tile, static, so the object states it; its 128
accumulator registers and the eight fp32 x vectors in flight leave it below the 256 registers a lane has at the two waves
per SIMD its 512 threads make, as DESIGN.md states.  The pack kernel beside it holds its 32 x 33 float tile."""
from test_build_resources_darknet_io import _built


def test_wide_head_kernels_are_built_without_spills_or_scratch():
    meta = _built("wide_head.o")
    assert len(meta) == 2, sorted(meta)
    (name,) = [m for m in meta if "wide_head_forward_kernel" in m]
    r = meta[name]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 2 * (256 + 256) * 128 == 131072, r
    assert 128 < r["vgpr_count"] <= 256, r        # 128 accumulators and more; one workgroup of 8 waves per CU fits
    (pack,) = [m for m in meta if "wide_head_pack_kernel" in m]
    p = meta[pack]
    assert p["vgpr_spill_count"] == 0 and p["sgpr_spill_count"] == 0 and p["private_segment_fixed_size"] == 0, p
    assert p["group_segment_fixed_size"] == 32 * 33 * 4 and p["vgpr_count"] <= 64, p
    print("wide head kernels: %r %r" % (r, p))
