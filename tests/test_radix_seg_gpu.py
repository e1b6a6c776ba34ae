"""The radix sort in its full form (kiss_radix_sort with a segment column and / or first_pos, kiss_amd/csrc/radix.hip)
against a stable host sort, through `kiss_hip_debug_radix_sort_seg`.

What the whole suffix sorts, the stage partition and the rank doubling otherwise reach only with whatever shapes their
texts happen to produce: k_radix_scatter<0, true, *> (key passes that carry the segment column), k_radix_scatter<1, true, *>
and k_radix_hist<1> (digits of the segment word), k_radix_hist_all<true> with every number of LDS histogram copies, the
key_lo_bit = 64 form without a key pass, first_pos including the count == 1 copy, and the segment column left alone at
seg_bits == 0.  Cases, the segment-value contract and the reference: tests/radix_seg_cases.py; that the cases can catch
an error: tests/test_radix_seg_cases.py (CPU).

Every case runs on the shipped library (one-sweep from two tiles on, tile histograms below) and once more in ONE child
process on the hooks build with KISS_HIP_NO_ONESWEEP=1 (tile histograms + matrix scan for every count): the child checks
its output against the same reference in full and hands back SHA-256 digests of the three columns, which have to be
those of the shipped library's output."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import radix_seg_cases as rs
from tests.radix_seg_cases import CASES, case_id

pytestmark = pytest.mark.gpu

MAX_N = 4_000_000  # m_cap = 0.32 * max_n + 4096 > 64 * 16384 + 1
E_INVALID = -1


def device_sort(ctx, lib, c, keys, seg, pos):
    k, s, p = keys.copy(), seg.copy(), pos.copy()
    rc = lib.kiss_hip_debug_radix_sort_seg(ctx._ctx, k.ctypes.data, s.ctypes.data, p.ctypes.data, k.size, c.key_lo_bit,
                                           c.seg_bits, c.flags)
    assert rc == 0, rc
    return k, s, p


def check(c, got, keys, seg, pos, order):
    k, s, p = got
    assert np.array_equal(p, pos[order]), "positions"
    assert np.array_equal(s, seg[order]), "segment column"
    assert np.array_equal(k, keys[order]), "keys (with the payload below the sorted bits)"


def digests(got):
    return [hashlib.sha256(a.tobytes()).hexdigest() for a in got]


def launches(lib, count):
    """(radix_hist, scan, radix_scatter) launches of one five-pass sort of `count` items, as the library's timers count them"""
    import kiss_amd
    c = rs.Case(count, 40, 9, "uniform", "uniform", 0)
    keys, seg, pos, order = rs.make_case(c)
    with kiss_amd.Context(max_n=400_000, device=0, profiling=True) as ctx:
        before = ctx.stats()["kernels"]
        check(c, device_sort(ctx, lib, c, keys, seg, pos), keys, seg, pos, order)
        after = ctx.stats()["kernels"]
    return [int(after[k]["launches"] - before[k]["launches"]) for k in ("radix_hist", "scan", "radix_scatter")]


def run_all_cases():
    """(child process) every case on the library the environment selects: checked in full, digests printed."""
    import kiss_amd
    lib = kiss_amd.load()
    assert lib.kiss_hip_has_hooks() == 1 and os.environ.get("KISS_HIP_NO_ONESWEEP")
    out = {}
    with kiss_amd.Context(max_n=MAX_N, device=0) as ctx:
        for c in CASES:
            keys, seg, pos, order = rs.make_case(c)
            got = device_sort(ctx, lib, c, keys, seg, pos)
            check(c, got, keys, seg, pos, order)
            out[case_id(c)] = digests(got)
    out["launches"] = launches(lib, 2 * rs.TILE + 1)
    print("DIGESTS " + json.dumps(out))


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=MAX_N, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tile_histogram_form():
    """Digests of every case without the one-sweep form: hooks build, KISS_HIP_NO_ONESWEEP=1, one fresh child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from tests import test_radix_seg_gpu as t; t.run_all_cases()"
    env = dict(os.environ, KISS_AMD_LIB="hooks", KISS_HIP_NO_ONESWEEP="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("DIGESTS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    got = json.loads(lines[0][len("DIGESTS "):])
    assert sorted(got) == sorted([case_id(c) for c in CASES] + ["launches"])  # the child ran every case
    return got


def test_the_two_runs_take_the_two_dispatch_forms(tile_histogram_form):
    import kiss_amd
    lib = kiss_amd.load()
    # one-sweep from two tiles on: ONE histogram launch for all five passes and no matrix scan ...
    assert launches(lib, 2 * rs.TILE + 1) == [1, 0, 5]
    # ... a single tile, and every count in the child: a histogram and a matrix scan in front of every scatter
    hist, scan, scatter = launches(lib, rs.TILE)
    assert (hist, scatter) == (5, 5) and scan >= 10
    hist, scan, scatter = tile_histogram_form["launches"]
    assert (hist, scatter) == (5, 5) and scan >= 10


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_segment_sort_is_stable_and_the_same_in_both_dispatch_forms(ctx, tile_histogram_form, c):
    import kiss_amd
    lib = kiss_amd.load()
    assert not os.environ.get("KISS_AMD_LIB") and not os.environ.get("KISS_AMD_LIB_PATH")  # the shipped library
    assert lib.kiss_hip_has_hooks() == 0
    keys, seg, pos, order = rs.make_case(c)
    got = device_sort(ctx, lib, c, keys, seg, pos)
    check(c, got, keys, seg, pos, order)
    assert digests(got) == tile_histogram_form[case_id(c)]


@pytest.mark.parametrize("c", [c for c in CASES if c.seg_bits == 0 and c.flags == 0], ids=case_id)
def test_without_segments_it_is_the_old_hook(ctx, c):
    import kiss_amd
    lib = kiss_amd.load()
    keys, seg, pos, order = rs.make_case(c)
    k0, p0 = keys.copy(), pos.copy()
    assert lib.kiss_hip_debug_radix_sort(ctx._ctx, k0.ctypes.data, p0.ctypes.data, k0.size, c.key_lo_bit) == 0
    k1, s1, p1 = device_sort(ctx, lib, c, keys, seg, pos)
    assert np.array_equal(k1, k0) and np.array_equal(p1, p0)
    # seg_bits == 0: the column of buffer 0 comes back, untouched whatever it holds, and may be left out altogether
    marks = (np.arange(keys.size, dtype=np.uint32) * np.uint32(7)) + np.uint32(3)
    k2, s2, p2 = device_sort(ctx, lib, c, keys, marks, pos)
    assert np.array_equal(s2, marks) and np.array_equal(k2, k0) and np.array_equal(p2, p0)
    k3, p3 = keys.copy(), pos.copy()
    assert lib.kiss_hip_debug_radix_sort_seg(ctx._ctx, k3.ctypes.data, None, p3.ctypes.data, k3.size, c.key_lo_bit, 0, 0) == 0
    assert np.array_equal(k3, k0) and np.array_equal(p3, p0)


def test_argument_checks(ctx):
    import kiss_amd
    lib = kiss_amd.load()
    k, s, p = np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.arange(4, dtype=np.uint32)

    def call(keys=k, seg=s, pos=p, count=4, lo=24, sb=8, flags=0, handle=ctx._ctx):
        ptr = [a.ctypes.data if a is not None else None for a in (keys, seg, pos)]
        return lib.kiss_hip_debug_radix_sort_seg(handle, ptr[0], ptr[1], ptr[2], count, lo, sb, flags)

    assert call() == 0
    assert call(handle=None) == E_INVALID and call(keys=None) == E_INVALID and call(pos=None) == E_INVALID
    assert call(seg=None) == E_INVALID and call(seg=None, sb=0) == 0
    assert call(lo=-1) == E_INVALID and call(lo=65) == E_INVALID and call(lo=64) == 0
    assert call(sb=-1) == E_INVALID and call(sb=33) == E_INVALID and call(lo=0, sb=32) == 0  # twelve passes: the most
    assert call(flags=2) == E_INVALID
    assert call(lo=64, sb=0, flags=1) == E_INVALID and call(lo=64, sb=0) == 0 and call(lo=64, sb=1, flags=1) == 0  # (no pass)
    cap = ctypes.c_uint64()
    ptr = ctypes.c_void_p()
    assert lib.kiss_hip_stage_view(ctx._ctx, 1, ctypes.byref(ptr), ctypes.byref(cap)) == 0 and cap.value >= rs.BIG_COUNT
    assert call(count=cap.value + 1) == E_INVALID  # (rejected before anything is read)
    assert np.array_equal(p, np.arange(4)) and not k.any() and not s.any()
