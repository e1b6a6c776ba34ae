"""k_fc0_onepass runs one 1024-thread workgroup per CU and every tile waits on its predecessors' descriptors: a register
spill or a register count past 128 (the workgroup would no longer fit a CU) shows nowhere at run time but in the time.
k_pair_finish is a chain of dependent text loads per lane and must not go through scratch either.  This test reads the
figures from the code-object metadata of the built library (kiss_amd/csrc/flag_compact.hip).  No GPU needed."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "kiss_amd", "libkiss_hip.so")
LLVM_BIN = "/opt/rocm/llvm/bin"

# a SIMD of gfx950 has 512 registers per lane (VGPRs and AGPRs share the file); a workgroup of 16 waves puts 4 on each
REGS_PER_SIMD_LANE = 512


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
    if not os.path.exists(LIB):
        pytest.skip("libkiss_hip.so is not built")
    found = _kernels(LIB, str(tmp_path_factory.mktemp("fc0_resources")))
    assert any("k_fc0_onepass" in n for n in found), "metadata not read: %d kernels" % len(found)
    return found


def _no_scratch(md):
    assert int(md["private_segment_fixed_size"]) == 0, md
    assert int(md["vgpr_spill_count"]) == 0 and int(md["sgpr_spill_count"]) == 0, md
    assert md["uses_dynamic_stack"] == "false", md


def test_fc0_onepass_fits_one_workgroup_per_cu_without_scratch(kernels):
    forms = {name: md for name, md in kernels.items() if "k_fc0_onepass" in name}
    assert len(forms) == 2, "k_fc0_onepass<with / without pair records>: %s" % sorted(forms)
    for name, md in forms.items():
        threads = int(md["max_flat_workgroup_size"])
        assert threads == 1024, (name, threads)
        _no_scratch(md)
        waves_per_simd = (threads // 64) // 4
        assert REGS_PER_SIMD_LANE // waves_per_simd == 128
        assert int(md["vgpr_count"]) + int(md["agpr_count"]) <= 128, (name, md)


def test_pair_finish_has_no_scratch(kernels):
    forms = [md for name, md in kernels.items() if "k_pair_finish" in name]
    assert len(forms) == 1, "k_pair_finish: %d kernels of that name in the library" % len(forms)
    _no_scratch(forms[0])
