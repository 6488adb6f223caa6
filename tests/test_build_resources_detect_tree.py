"""CPU test of the BUILT detect_tree.o (no GPU), resource metadata only: the walk kernel and the three detect kernels of
the word-tree detect path exist, spill nothing and own no scratch; the detect kernels stay within 128 VGPRs (their
workgroup is 1,024 lanes: four waves per SIMD) and hold only their one counter as static LDS; the walk kernel has no LDS
at all.  detect.o, darknet_io.o and word_tree.o, which lent helper functions to headers, hold the kernels they held."""
from test_build_resources_darknet_io import _built


def _clean(name, r):
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)


def test_detect_tree_kernels_are_built_without_spills_or_scratch():
    meta = _built("detect_tree.o")
    # detect_anchor_tree_kernel<false> (stretch) and <true> (letterbox), the Darknet rows, the walk
    words = ("word_tree_top_kernel", "detect_anchor_tree_kernelILb0E", "detect_anchor_tree_kernelILb1E",
             "detect_anchor_tree_dk_kernel")
    assert len(meta) == len(words), sorted(meta)
    for word in words:
        (name,) = [m for m in meta if word in m]
        r = meta[name]
        _clean(name, r)
        if word == "word_tree_top_kernel":
            assert r["group_segment_fixed_size"] == 0, (name, r)           # no LDS: the node limit is index arithmetic's
            assert r["vgpr_count"] <= 64, (name, r)                        # a wave per row: full occupancy
        else:
            assert r["vgpr_count"] <= 128, (name, r)
            assert r["group_segment_fixed_size"] <= 16, (name, r)          # s_valid; the sort slots are dynamic
    print("detect_tree kernels: %r" % (meta,))


def test_the_files_that_lent_their_helpers_hold_the_kernels_they_held():
    held = {"detect.o": ("detect_grid_kernel", "detect_anchor_kernelILb0E", "detect_anchor_kernelILb1E",
                         "detect_anchor_classes_kernelILb0E", "detect_anchor_classes_kernelILb1E",
                         "voc_match_kernelILb0E"),
            "darknet_io.o": ("letterbox_darknet_kernel", "detect_anchor_classes_dk_kernel", "voc_match_kernelILb1E"),
            "word_tree.o": ("yolov2_loss_boxes_tree_kernel", "yolov2_loss_boxes_tree_finalize_kernel",
                            "yolov2_region_stats_tree_kernel", "yolov2_region_stats_tree_finalize_kernel",
                            "word_tree_head_kernel")}
    for obj, words in held.items():
        meta = _built(obj)
        assert len(meta) == len(words), (obj, sorted(meta))
        for word in words:
            (name,) = [m for m in meta if word in m]
            _clean(name, meta[name])
