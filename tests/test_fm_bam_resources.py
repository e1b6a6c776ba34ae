"""The BAM kernels keep what they know of a record in registers: no scratch and no spills, scalar ones included, and LDS only
where the framing kernel stages a block and keeps its CRC table.  This test reads the figures from the code-object metadata of the
built library (kiss_amd/csrc/fm_bam.hip), as tests/test_fm_pileup_resources.py does.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_bam_count", "k_bam_size", "k_bam_emit", "k_bgzf")
BGZF_LDS = 4 * 256 + 4 * 16384 + 4  # the CRC table, a block of 65505 bytes at any byte phase, the word the waves XOR into
LDS_PER_CU = 160 << 10


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fm_bam_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_bam_kernels_have_no_scratch_no_spills_and_lds_only_in_the_framing(kernels):
    for kernel in KERNELS:
        mangled = "%d%sE" % (len(kernel), kernel)
        forms = {name: md for name, md in kernels.items() if mangled in name}
        assert len(forms) == 1, "%s: %s" % (kernel, sorted(forms))
        (name, md), = forms.items()
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                         "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["group_segment_fixed_size"]) == (BGZF_LDS if kernel == "k_bgzf" else 0), md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE // MIN_WAVES_PER_SIMD, md
    assert 2 * BGZF_LDS <= LDS_PER_CU < 3 * BGZF_LDS  # two framing workgroups, eight waves, share a CU


def test_the_sam_kernels_that_bam_shares_are_the_units_own(kernels):
    """k_sam_head and k_sam_check come from fm_sam_line.hpp into both units: two copies, neither with scratch"""
    for kernel in ("k_sam_head", "k_sam_check"):
        forms = [md for name, md in kernels.items() if "%d%sE" % (len(kernel), kernel) in name]
        assert forms and all(int(md["private_segment_fixed_size"]) == 0 and int(md["sgpr_spill_count"]) == 0 for md in forms), kernel
