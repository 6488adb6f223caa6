"""CPU test of the BUILT augment.o (no GPU), resource metadata only: the box-list kernel with the draw exists once, spills
nothing, owns no scratch -- its ballot words are 128 bytes of LDS, one bit per object up to Y2_DRAW_MAX_OBJ, not an indexed
per-thread array -- and stays at full occupancy (at most 64 VGPRs), as DESIGN.md states; the kernel without the draw beside
it keeps no LDS and no scratch."""
from test_build_resources_darknet_io import _built


def test_box_list_draw_kernel_is_built_without_spills_or_scratch():
    meta = _built("augment.o")
    (name,) = [m for m in meta if "encode_box_list_draw_kernel" in m]
    r = meta[name]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] == 1024 // 64 * 8, r
    (plain,) = [m for m in meta if "encode_box_list_kernel" in m]
    p = meta[plain]
    assert p["vgpr_spill_count"] == 0 and p["private_segment_fixed_size"] == 0 and p["group_segment_fixed_size"] == 0, p
    print("box list kernels: %r %r" % (r, p))
