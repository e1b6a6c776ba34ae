"""The rescue plan walks one wave per pair and keeps a lane's window and its two running chain counts in registers between
the ballots; the merge kernels are one lane per record or op.  Scratch or spills would put that state into memory.  This
test reads the figures from the code-object metadata of the built library (kiss_amd/csrc/fm_rescue.hip), as
tests/test_fm_pair_resources.py does for k_mate_walk.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_rescue_head", "k_rescue_count", "k_rescue_emit", "k_rescue_merge_head", "k_rescue_merge_place", "k_rescue_merge_emit",
           "k_rescue_merge_ops")
OTHER_FAMILIES = ("k_mate_", "k_select_", "k_align_")  # (the resource tests of those calls pick their kernels by these)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fm_rescue_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def _one(kernels, kernel):
    mangled = "%d%sE" % (len(kernel), kernel)  # (the whole name: k_rescue_head is no k_rescue_merge_head)
    forms = {name: md for name, md in kernels.items() if mangled in name}
    assert len(forms) == 1, "%s: %s" % (kernel, sorted(forms))
    (name, md), = forms.items()
    return name, md


def test_rescue_kernels_have_no_scratch_no_spills_no_dynamic_stack(kernels):
    names = sorted(n for n in kernels if "k_rescue_" in n)
    assert len(names) == len(KERNELS), names
    for name in names:
        assert not any(f in name for f in OTHER_FAMILIES), name
    for kernel in KERNELS:
        name, md = _one(kernels, kernel)
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                         "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["group_segment_fixed_size"]) == 0, md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE // MIN_WAVES_PER_SIMD, md
