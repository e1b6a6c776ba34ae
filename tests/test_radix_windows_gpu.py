"""The windowed radix scatter (k_radix_scatter_win, kiss_amd/csrc/radix.hip) against numpy's stable sort and against
the one-buffer kernel it replaces on large inputs.

`kiss_hip_debug_radix_sort` with key_lo_bit = 24 runs the round-0 shape: five passes over (key64, pos32).  A pass goes
to the windowed kernel when it has at least 513 tiles of 16384 items (RX_WIN_MIN_TILES), so of the counts below those
>= 16384 * 513 - 1 reach it on the shipped library (16384 * 513 + {-1, 0, 1} and 10 000 019) and the smaller ones check
that the dispatch leaves them where they were.  Every case also runs in a child process on the hooks build with
KISS_HIP_RX_ONE_TILE=1, which sends every pass to the old kernel: the child checks its output against the same
numpy reference in full and hands back SHA-256 digests of the key and position bytes, which have to be those of the
shipped library's output."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384
MAX_N = 32 * 1024 * 1024  # m_cap = 0.32 * max_n > 10 000 019
COUNTS = ([TILE * t + e for t in (1, 2, 3, 64, 513) for e in (-1, 0, 1)]
          + [TILE + 4096 * q + e for q in (1, 2, 3) for e in (-1, 0, 1)] + [10_000_019])
KINDS = ["uniform", "one_digit", "split_at_window", "split_off_by_one", "geometric", "sorted", "reverse"]
LO_BIT = 24


def make_keys(kind, n):
    """Keys whose five digits (bits 24..63) follow `kind`; the low 24 bits are random payload that has to travel."""
    rng = np.random.default_rng([KINDS.index(kind), n])
    low = rng.integers(0, 1 << 24, n, dtype=np.uint64)
    if kind == "uniform":
        return rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | (low & np.uint64(1))
    if kind == "one_digit":  # one run through every window, in every pass
        return np.uint64(0x5A17C3E9A1 << 24) | low
    if kind in ("split_at_window", "split_off_by_one"):
        # two digits per tile; the first one ends exactly at (one slot off) a quarter of the tile, another quarter from
        # tile to tile, in the first pass (bits 24..31) -- and, the other digits being equal, nothing moves after it
        i = np.arange(n, dtype=np.uint64)
        tile, off = i // np.uint64(TILE), i % np.uint64(TILE)
        cut = np.uint64(4096) * (np.uint64(1) + tile % np.uint64(3))
        if kind == "split_off_by_one":
            cut = np.where(tile % np.uint64(2) == 0, cut + np.uint64(1), cut - np.uint64(1))
        digit = np.where(off < cut, np.uint64(0x21), np.uint64(0xC4))
        return np.uint64(0x0102030400 << 24) | (digit << np.uint64(24)) | low
    if kind == "geometric":  # a few long runs and many runs of one item, independently in every digit
        k = np.zeros(n, dtype=np.uint64)
        for b in range(5):
            d = np.minimum(rng.geometric(0.04, n) - 1, 255).astype(np.uint64)
            k |= d << np.uint64(24 + 8 * b)
        return k | low
    u = np.sort(rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1))
    return u if kind == "sorted" else u[::-1].copy()


def reference(keys):
    order = np.argsort(keys >> np.uint64(LO_BIT), kind="stable").astype(np.uint32)
    return keys[order], order


def device_sort(ctx, lib, keys):
    k = np.ascontiguousarray(keys, dtype=np.uint64).copy()
    p = np.arange(k.size, dtype=np.uint32)
    rc = lib.kiss_hip_debug_radix_sort(ctx._ctx, k.ctypes.data, p.ctypes.data, k.size, LO_BIT)
    assert rc == 0, rc
    return k, p


def digests(k, p):
    return [hashlib.sha256(k.tobytes()).hexdigest(), hashlib.sha256(p.tobytes()).hexdigest()]


def run_all_cases():
    """(child process) every case on the library the environment selects: checked in full, digests printed."""
    import kiss_amd
    lib = kiss_amd.load()
    out = {}
    with kiss_amd.Context(max_n=MAX_N, device=0) as ctx:
        for kind in KINDS:
            for n in COUNTS:
                keys = make_keys(kind, n)
                k, p = device_sort(ctx, lib, keys)
                want_k, want_p = reference(keys)
                assert np.array_equal(p, want_p) and np.array_equal(k, want_k), (kind, n)
                out["%s/%d" % (kind, n)] = digests(k, p)
    print("DIGESTS " + json.dumps(out))


@pytest.fixture(scope="module")
def ctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=MAX_N, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def one_tile_form():
    """Digests of every case from the old kernel: hooks build, KISS_HIP_RX_ONE_TILE=1, one child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from tests import test_radix_windows_gpu as t; t.run_all_cases()"
    env = dict(os.environ, KISS_AMD_LIB="hooks", KISS_HIP_RX_ONE_TILE="1", PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [line for line in r.stdout.splitlines() if line.startswith("DIGESTS ")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0][len("DIGESTS "):])


def test_the_cases_are_what_they_claim():
    # (no device work) the split cases really end a digit at / one slot off a quarter of the tile
    for kind, slack in (("split_at_window", 0), ("split_off_by_one", 1)):
        keys = make_keys(kind, 4 * TILE)
        d = (keys >> np.uint64(24)) & np.uint64(255)
        for t in range(4):
            first = int(np.count_nonzero(d[t * TILE:(t + 1) * TILE] == 0x21))
            assert abs(first - 4096 * (1 + t % 3)) == slack, (kind, t, first)
    assert max(COUNTS) <= int(0.32 * MAX_N) and sum(1 for n in COUNTS if -(-n // TILE) >= 513) == 4


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_windowed_scatter_sorts_stably_and_like_the_one_tile_form(ctx, one_tile_form, kind, n):
    import kiss_amd
    assert not os.environ.get("KISS_AMD_LIB") and not os.environ.get("KISS_AMD_LIB_PATH")  # the shipped library
    keys = make_keys(kind, n)
    k, p = device_sort(ctx, kiss_amd.load(), keys)
    want_k, want_p = reference(keys)
    assert np.array_equal(p, want_p)
    assert np.array_equal(k, want_k)
    assert digests(k, p) == one_tile_form["%s/%d" % (kind, n)]
