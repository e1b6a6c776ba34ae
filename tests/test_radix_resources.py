"""The windowed radix scatter only pays while TWO of its workgroups fit a CU (kiss_amd/csrc/radix.hip,
DESIGN.md 4.0).  Nothing at run time says when a later edit has pushed it back to one workgroup per CU or into
scratch, so this test reads the figures from the code-object metadata of the built library.  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kiss_amd", "libkiss_hip.so")
LLVM_BIN = "/opt/rocm/llvm/bin"

# a CU of gfx950: 160 KiB of LDS, 512 registers per lane and SIMD; a workgroup of 16 waves puts 4 waves on each SIMD
LDS_PER_CU = 160 * 1024
REGS_PER_SIMD_LANE = 512
WORKGROUPS_PER_CU = 2


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


@pytest.mark.skipif(not os.path.exists(LIB), reason="libkiss_hip.so is not built")
def test_windowed_scatter_fits_two_workgroups_per_cu_without_scratch(tmp_path):
    kernels = _kernels(LIB, str(tmp_path))
    assert any("k_radix_scatterI" in n for n in kernels), "metadata not read: %d kernels" % len(kernels)
    win = [md for name, md in kernels.items() if "k_radix_scatter_win" in name]
    assert len(win) == 1, "k_radix_scatter_win: %d kernels of that name in the library" % len(win)
    md = win[0]
    threads = int(md["max_flat_workgroup_size"])
    assert threads == 1024, threads
    # no scratch: spilling forms of the hot kernels have lost every time they were measured
    assert int(md["private_segment_fixed_size"]) == 0, md
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
    assert md["uses_dynamic_stack"] == "false", md
    # two workgroups per CU: LDS and registers (VGPRs and AGPRs share one file on gfx950)
    assert int(md["group_segment_fixed_size"]) <= LDS_PER_CU // WORKGROUPS_PER_CU == 81920, md
    waves_per_simd = WORKGROUPS_PER_CU * (threads // 64) // 4
    budget = REGS_PER_SIMD_LANE // waves_per_simd
    assert budget == 64
    assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= budget, md
