"""CPU test of the BUILT coco.o (no GPU), resource metadata only: the one kernel of COCO's matching exists, spills nothing,
owns no scratch -- its per-lane "matched" set is bytes in LDS, not an indexed per-thread array -- stays at full occupancy
(at most 64 VGPRs) and holds no static LDS (its 116 bytes per slot of the box table are dynamic), as DESIGN.md states."""
from test_build_resources_darknet_io import _built


def test_coco_match_kernel_is_built_without_spills_or_scratch():
    meta = _built("coco.o")
    assert len(meta) == 1 and "coco_match_kernel" in list(meta)[0], sorted(meta)
    (r,) = meta.values()
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["vgpr_count"] <= 64 and r["group_segment_fixed_size"] == 0, r
    print("coco kernel: %r" % (meta,))
