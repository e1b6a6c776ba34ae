"""k_mate_walk runs one wave per pair and keeps the first chunk of either mate and the best combination of every lane in
registers between its two sweeps: scratch or spills would put them into memory and every shuffle step behind a load.  This
test reads the figures from the code-object metadata of the built library (kiss_amd/csrc/fm_pair.hip), as
tests/test_fm_select_resources.py does for k_select_walk.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, MIN_WAVES_PER_SIMD, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_mate_head", "k_mate_walk")
WALK_VGPRS = 92  # five waves per SIMD


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fm_pair_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_pair_kernels_have_no_scratch_no_spills_no_dynamic_stack(kernels):
    names = sorted(n for n in kernels if "k_mate_" in n)
    assert len(names) == len(KERNELS), names
    for kernel in KERNELS:
        forms = {name: md for name, md in kernels.items() if kernel in name}
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


def test_the_walk_keeps_the_register_count_the_design_quotes(kernels):
    (md,) = [md for name, md in kernels.items() if "k_mate_walk" in name]
    assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= WALK_VGPRS, md
