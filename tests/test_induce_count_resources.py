"""The count pass of the induction (k_induce_count, kiss_amd/csrc/induce.hip) is a stream of loads with little work per
byte: it hides their round trip behind other waves, so it only pays at EIGHT waves per SIMD -- 64 registers -- and without
scratch.  Before the refresh path became a loop it needed 112 registers and ran at half that occupancy; nothing at run time
but the time shows such a relapse, so this test reads the figures from the code-object metadata of the built library
(DESIGN.md 4), as tests/test_radix_resources.py does for the radix scatter.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, REGS_PER_SIMD_LANE, _kernels

WAVES_PER_SIMD = 8


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("induce_count_resources")))
    assert any("k_induce_scatter" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_both_count_kernels_fit_eight_waves_per_simd_without_scratch(kernels):
    forms = {name: md for name, md in kernels.items() if "k_induce_count" in name}
    # k_induce_count<true> (the LMS passes: context words of the far list) and <false> (class bytes beside SA)
    assert sorted("ILb1E" in n for n in forms) == [False, True], "k_induce_count: %s" % sorted(forms)
    budget = REGS_PER_SIMD_LANE // WAVES_PER_SIMD
    assert budget == 64
    for name, md in sorted(forms.items()):
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= budget, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        assert int(md["group_segment_fixed_size"]) == 0, md  # no LDS: nothing else limits the waves of a CU
