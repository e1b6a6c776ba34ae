"""The pileup walk keeps its state -- the positions in read and text and the nine sums of the report -- in wave-uniform
registers between the adds.  Scratch, spills or LDS would put that state into memory.  This test reads the figures from the
code-object metadata of the built library (kiss_amd/csrc/fm_pileup.hip), as tests/test_fm_md_resources.py does
for the MD kernels.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_pile_head", "k_pile_check_ops", "k_pile_zero", "k_pile_walk")


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fm_pileup_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_pileup_kernels_have_no_scratch_no_spills_no_lds(kernels):
    names = sorted(n for n in kernels if "k_pile_" in n)
    assert len(names) == len(KERNELS), names
    for kernel in KERNELS:
        mangled = "%d%sE" % (len(kernel), kernel)
        forms = {name: md for name, md in kernels.items() if mangled in name}
        assert len(forms) == 1, "%s: %s" % (kernel, sorted(forms))
        (name, md), = forms.items()
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                         "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["group_segment_fixed_size"]) == 0, md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE // MIN_WAVES_PER_SIMD, md
