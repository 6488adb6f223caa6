"""CPU test of the BUILT darknet_io.o and detect.o (no GPU), resource metadata only: the three kernels of Darknet's
test-time protocol exist, spill nothing, own no scratch, stay at full occupancy (at most 64 VGPRs: 8 waves per SIMD) and
hold the static LDS DESIGN.md states (the image kernel and the matcher none; the detect kernel its one counter, its sort
slots being dynamic: 25 bytes per slot).  The matcher is one template with the integer rows' kernel of detect.o, whose
figures are the ones it had as a plain kernel."""
import os
import re
import struct
import subprocess

import pytest

from test_build_resources import LLVM, ROOT


def _kernel_notes(obj):
    """{kernel name: {metadata key: int}} of the gfx950 code object inside `obj`, from the notes alone"""
    tmp = obj + ".fatbin.tmp"
    try:
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", obj, tmp],
                       check=True)
        d = open(tmp, "rb").read()
        assert d.startswith(b"__CLANG_OFFLOAD_BUNDLE__")
        n = struct.unpack_from("<Q", d, 24)[0]
        off, co = 32, None
        for _ in range(n):
            o, sz, tl = struct.unpack_from("<QQQ", d, off)
            off += 24
            triple = d[off:off + tl].decode()
            off += tl
            if "gfx950" in triple:
                co = d[o:o + sz]
        assert co is not None, "no gfx950 code object in " + obj
        open(tmp, "wb").write(co)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", tmp], check=True, capture_output=True,
                               text=True).stdout
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    out = {}
    for block in notes.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            keys = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                    "group_segment_fixed_size")
            out[name.group(1)] = {k: int(re.search(r"\.%s:\s+(\S+)" % k, block).group(1)) for k in keys}
    return out


def _built(name):
    obj = os.path.join(ROOT, "tensorflow_yolo2_amd", "csrc", name)
    if not (os.path.exists(obj) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))):
        pytest.skip("%s not built here (run __graft_entry__.build())" % name)
    return _kernel_notes(obj)


def test_darknet_io_kernels_are_built_without_spills_or_scratch():
    meta = _built("darknet_io.o")
    static_lds = {"letterbox_darknet_kernel": 0, "detect_anchor_classes_dk_kernel": 16, "voc_match_kernelILb1E": 0}
    assert len(meta) == 3, sorted(meta)
    for word, lds in static_lds.items():
        (name,) = [m for m in meta if word in m]
        r = meta[name]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (name, r)
        assert r["vgpr_count"] <= 64, (name, r)
        assert r["group_segment_fixed_size"] == lds, (name, r)
    print("darknet_io kernels: %r" % (meta,))


def test_the_integer_matcher_keeps_its_figures_as_a_template_instance():
    meta = _built("detect.o")
    (name,) = [m for m in meta if "voc_match_kernel" in m]
    assert "ILb0E" in name, name
    r = meta[name]
    assert r["vgpr_count"] == 60 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] == 0, r
