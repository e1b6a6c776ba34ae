"""The kernels of the duplicate marking keep what they know in registers: workgroups of 256, no scratch, no spills, scalar ones
included, no dynamic stack, and no LDS at all -- the long cigars and quals of a wave are summed across its lanes by shuffles, not
through memory.  This test reads the figures from the code-object metadata of the built library (kiss_amd/csrc/bam_markdup.hip,
DESIGN.md 4.26), as tests/test_bam_sort_resources.py does.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_mk_record", "k_mk_class", "k_mk_items", "k_mk_key", "k_mk_heads", "k_mk_mark")
LDS = 0  # bytes, every kernel


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("markdup_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_markdup_kernels_have_no_scratch_no_spills_and_no_lds(kernels):
    for kernel in KERNELS:
        mangled = "%d%sE" % (len(kernel), kernel)
        forms = {name: md for name, md in kernels.items() if mangled in name}
        assert len(forms) == 1, "%s: %s" % (kernel, sorted(forms))
        (name, md), = forms.items()
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                         "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["group_segment_fixed_size"]) == LDS, md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE // MIN_WAVES_PER_SIMD, md
