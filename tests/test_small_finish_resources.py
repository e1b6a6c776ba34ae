"""k_small_finish keeps a window of the survivor stream in LDS and its lanes walk pairs of suffixes through the text, chains
of dependent loads: scratch, or fewer than four waves per SIMD to hide those loads behind, shows nowhere at run time but in
the time.  This test reads the figures from the code-object metadata of the built library (kiss_amd/csrc/lms_sort.hip,
DESIGN.md 4), as tests/test_fc0_resources.py does for k_fc0_onepass (flag_compact.hip).  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kiss_amd", "libkiss_hip.so")
LLVM_BIN = "/opt/rocm/llvm/bin"

# a SIMD of gfx950 has 512 registers per lane (VGPRs and AGPRs share the file): four waves get 128 each
REGS_PER_SIMD_LANE = 512
MIN_WAVES_PER_SIMD = 4


def _kernels(lib, workdir):
    """{kernel name: {metadata key: value}} over every gfx950 code object inside `lib`."""
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    assert os.path.exists(objdump) and os.path.exists(readelf), "llvm-objdump / llvm-readelf not found in " + LLVM_BIN
    copy = os.path.join(workdir, "lib.so")  # (the bundles are extracted beside the file that is read)
    shutil.copy(lib, copy)
    subprocess.run([objdump, "--offloading", copy], cwd=workdir, check=True, capture_output=True, timeout=300)
    out = {}
    for f in sorted(os.listdir(workdir)):
        if "gfx950" not in f:
            continue
        notes = subprocess.run([readelf, "--notes", os.path.join(workdir, f)], check=True, capture_output=True,
                               text=True, timeout=300).stdout
        cur = None
        for line in notes.splitlines():
            if re.match(r"^  - \.", line):  # first key of the next kernel
                cur = {}
                line = "    " + line[4:]
            elif re.match(r"^\S", line):
                cur = None
            m = re.match(r"^    \.([a-z_]+):\s+(\S.*)$", line)
            if cur is not None and m:
                cur[m.group(1)] = m.group(2).strip()
                if m.group(1) == "name":
                    out[m.group(2).strip()] = cur
    return out


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    assert os.path.exists(LIB), "libkiss_hip.so is not built"
    found = _kernels(LIB, str(tmp_path_factory.mktemp("small_finish_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def test_small_finish_has_no_scratch_and_four_waves_per_simd(kernels):
    forms = {name: md for name, md in kernels.items() if "k_small_finish" in name}
    assert len(forms) == 1, "k_small_finish: %s" % sorted(forms)
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
