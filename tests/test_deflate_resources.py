"""The kernels of kiss_amd/csrc/bgzf_deflate.hip keep a block's chain in LDS and registers: no scratch, no vector or scalar spills,
and the LDS of the block kernel is the figure DESIGN.md 4.23 states, which lets one workgroup (four waves) live on a CU.  Read from
the code-object metadata of the built library, as tests/test_fm_bam_resources.py does.  No GPU needed."""
import os

import pytest

from tests.test_small_finish_resources import LIB, REGS_PER_SIMD_LANE, _kernels

KERNELS = ("k_deflate_block", "k_deflate_pack")
BLOCK_LDS = 108960          # the payload 65552, the hash table 32768, the CRC table 1024, the code tables and the rest 9616
LDS_PER_CU = 160 << 10


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("deflate_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_deflate_kernels_have_no_scratch_and_no_spills(kernels):
    for kernel in KERNELS:
        mangled = "%d%sE" % (len(kernel), kernel)
        forms = {name: md for name, md in kernels.items() if mangled in name}
        assert len(forms) == 1, "%s: %s" % (kernel, sorted(forms))
        (name, md), = forms.items()
        print(name, {k: md[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size",
                                         "private_segment_fixed_size") if k in md})
        assert int(md["max_flat_workgroup_size"]) == 256, md
        assert int(md["private_segment_fixed_size"]) == 0, md
        assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
        assert md["uses_dynamic_stack"] == "false", md
        lds = int(md["group_segment_fixed_size"])
        if kernel == "k_deflate_block":
            assert lds <= BLOCK_LDS, md
            assert lds <= LDS_PER_CU < 2 * lds  # one workgroup a CU, as 4.23 says: one wave on every SIMD
            assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= REGS_PER_SIMD_LANE, md
        else:
            assert lds == 0, md
