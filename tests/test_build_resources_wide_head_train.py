"""CPU test of the BUILT wide_head_train.o (no GPU), resource metadata only: the six kernels of the wide head's training
exist once, spill nothing and own no scratch.  The two product kernels hold two stages of (128 + 128) rows x 128 bytes =
64 KiB of static LDS, so two workgroups share a CU's 160 KiB, and they stay within the 256 registers a lane has at the two
waves per SIMD those two 256-thread workgroups make: 64 accumulators, 32 operand values in flight in the data gradient and
64 in the filter gradient, the addresses ("Training the wide head").  The update holds its 32 x 33 float tile
as wide_head.hip's pack kernel does, the bias gradient its 8 x 32 partial sums; the streaming kernels stay at full
occupancy (at most 64 registers)."""
from test_build_resources_darknet_io import _built


def test_wide_head_train_kernels_are_built_without_spills_or_scratch():
    meta = _built("wide_head_train.o")
    assert len(meta) == 6, sorted(meta)
    budget = {"wide_head_dgrad_kernel": (65536, 64 + 32, 256), "wide_head_wgrad_kernel": (65536, 64 + 64, 256),
              "wide_head_sum_kernel": (0, 1, 64), "wide_head_db_kernel": (8 * 32 * 4, 1, 64),
              "wide_head_pack2_kernel": (0, 1, 64), "wide_head_sgd_kernel": (32 * 33 * 4, 1, 64)}
    for word, (lds, vgpr_above, vgpr_max) in budget.items():
        (name,) = [m for m in meta if word in m]
        r = meta[name]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["group_segment_fixed_size"] == lds, (name, r)
        assert vgpr_above < r["vgpr_count"] <= vgpr_max, (name, r)
    print("wide head training kernels: %r" % (meta,))
