"""k_align_dp runs one wave per chain and keeps the row above, per diagonal, in LDS: scratch, spills, or fewer than four
waves per SIMD to hide the LDS and shuffle latency behind, show nowhere at run time but in the time.  This test reads the
figures from the code-object metadata of the built library (kiss_amd/csrc/fm_align.hip), as
tests/test_small_finish_resources.py does for k_small_finish.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fm_align_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_align_dp_has_no_scratch_and_four_waves_per_simd(kernels):
    forms = {name: md for name, md in kernels.items() if "k_align_dp" in name}
    assert len(forms) == 1, "k_align_dp: %s" % sorted(forms)
    (name, md), = forms.items()
    print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                     "private_segment_fixed_size") if k in md})
    assert int(md["max_flat_workgroup_size"]) == 256, md
    assert int(md["private_segment_fixed_size"]) == 0, md
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
    assert md["uses_dynamic_stack"] == "false", md
    assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE // MIN_WAVES_PER_SIMD, md
    # LDS: 160 KiB per CU; four waves per SIMD are four workgroups of 256 threads per CU
    assert 4 * int(md["group_segment_fixed_size"]) <= 160 * 1024, md


def test_the_walks_have_no_scratch_either(kernels):
    for kernel in ("k_align_trace", "k_align_emit", "k_align_prep", "k_align_head"):
        forms = [md for name, md in kernels.items() if kernel in name]
        assert len(forms) == 1, kernel
        assert int(forms[0]["private_segment_fixed_size"]) == 0 and forms[0]["uses_dynamic_stack"] == "false", (kernel, forms[0])
