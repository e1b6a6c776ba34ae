"""CPU checks of the any-SA_INTV / LOOKUP_LEN FM-index: the numpy model (tests/fm_model.py) against the C oracle at the
CLI's instantiation (4, 0), the layout of SA_INTV = 1, the lookup identity, and the new C-ABI entry points as far as they
need no device."""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

from kiss_amd import _lib
from tests import gen
from tests.fm_model import FmModel, expected_counts, lookup_of, sections
from tests.fmi_layout import canonical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["kiss_hip_fmi_sizes_ex_for", "kiss_hip_fmi_build_ex_dev", "kiss_hip_fmi_query_ex_dev",
               "kiss_hip_fmi_build_ex_host", "kiss_hip_fmi_query_ex_host"]


def texts():
    rng = np.random.default_rng(5)
    p3 = gen.periodic(30_000, 3, 1)
    p37 = gen.periodic(30_000, 37, 2, mutations=20)
    mixed = gen.iid(40_000, 9)
    mixed[5_000:15_000] = np.tile(rng.integers(0, 4, 7, dtype=np.uint8), 1429)[:10_000]
    mixed[20_000:26_000] = 3
    return {"iid": gen.iid(20_000, 3), "genome": gen.genome_like(60_000, 4), "period3": p3, "period37": p37,
            "mixed_repeats": mixed}


def patterns_of(S, Q, L, seed):
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, S.size - L, Q)
    pats = S[pos[:, None] + np.arange(L)[None, :]].copy()
    mut = rng.random(Q) < 0.2
    col = rng.integers(0, L, Q)
    pats[mut, col[mut]] = (pats[mut, col[mut]] + 1) % 4
    return np.ascontiguousarray(pats, dtype=np.uint8)


@pytest.mark.parametrize("name", ["iid", "genome", "period3", "period37", "mixed_repeats"])
def test_model_4_0_equals_the_oracle(oracle, name):
    S = texts()[name]
    SA = oracle.suffix_sort(S, 32)
    ref = oracle.fm_build(S, SA)
    m = FmModel(S, SA, 4, 0)
    assert canonical(m.serialize()) == canonical(ref.serialize())
    for L in (1, 5, 12, 32):
        pats = patterns_of(S, 300, L, L)
        a = m.query_batch(pats)
        b = ref.query_batch(pats)
        assert np.array_equal(a["beg"], b["beg"]) and np.array_equal(a["end"], b["end"])
        assert a["total_hits"] == b["total_hits"] and a["checksum"] == b["checksum"]
        assert np.array_equal(a["offsets_index"], b["offsets_index"])
        assert np.array_equal(a["offsets"], b["offsets"])


@pytest.mark.parametrize("sa_intv,lookup_len", [(1, 0), (1, 3), (2, 5), (3, 1), (8, 4), (32, 2)])
def test_layout_counts(oracle, sa_intv, lookup_len):
    S = gen.genome_like(10_000, 8)
    m = FmModel(S, oracle.suffix_sort(S, 32), sa_intv, lookup_len)
    buf = m.serialize()
    sec, N = sections(buf, sa_intv)
    assert N == S.size + 1
    assert {k: v[1] for k, v in sec.items()} == expected_counts(N, sa_intv, lookup_len)
    if sa_intv == 1:  # the whole SA, and no b_ / b_occ_ sections at all
        off, count, _ = sec["sa"]
        assert np.array_equal(np.frombuffer(buf, "<u4", count, off), oracle.suffix_sort(S, 32))
        with pytest.raises(struct.error):  # read as an SA_INTV != 1 file it runs out of bytes
            sections(buf, 4)


@pytest.mark.parametrize("name", ["period3", "period37", "mixed_repeats", "genome"])
def test_lookup_identity(oracle, name):
    # the reference writes lookup_[2j + 1] = end(2j): the table must equal beg(K) for every K whatever the batching
    S = texts()[name]
    m = FmModel(S, oracle.suffix_sort(S, 32), 4, 6)
    keys = np.arange(4 ** 6)
    beg, end = m.search_keys(keys, 6)
    assert np.array_equal(m.lookup[:-1], beg.astype(np.uint32))
    assert np.array_equal(m.lookup[1:-1:2], end[0::2].astype(np.uint32))
    assert m.lookup[-1] == m.N
    assert lookup_of(m.serialize(), 4).tolist() == m.lookup.tolist()


def test_lookup_prologue_against_plain_search(oracle):
    # get_range through the table: lookup_[K + 1] is beg(K + 1), which equals end(K) when K and K + 1 differ only in the
    # last character (K % 4 != 3); for a key ending in T the reference's range may reach past end(K) (the rows between
    # are suffixes that do not extend K), and the model keeps that
    S = texts()["mixed_repeats"]
    SA = oracle.suffix_sort(S, 32)
    plain, tab = FmModel(S, SA, 4, 0), FmModel(S, SA, 4, 7)
    for L in (3, 7, 8, 20):
        pats = patterns_of(S, 500, L, 40 + L)
        a, b = plain.get_ranges(pats), tab.get_ranges(pats)
        if L < 7:  # no table
            assert all(np.array_equal(x, y) for x, y in zip(a, b))
            continue
        hit = a[1] > a[0]
        assert np.array_equal(a[0][hit], b[0][hit]) and (b[1][hit] >= a[1][hit]).all()
        if L == 7:  # the table alone: exact unless the key ends in T
            exact = hit & (pats[:, 6] != 3)
            assert np.array_equal(a[1][exact], b[1][exact])


def test_stop_cnt_rule(oracle):
    S = texts()["period3"]
    m = FmModel(S, oracle.suffix_sort(S, 32), 4, 2)
    pats = patterns_of(S, 200, 12, 4)
    beg0, end0, offs0 = m.get_ranges(pats, 0)
    assert (offs0[end0 > beg0] == 0).all()
    begx, endx, offsx = m.get_ranges(pats, 0xFFFFFFFF)  # stop_cnt + 1 wraps to 0: never stops, even on an empty range
    hit = end0 > beg0
    assert np.array_equal(begx[hit], beg0[hit]) and np.array_equal(endx[hit], end0[hit])
    assert np.array_equal(endx - begx, end0 - beg0) and (offsx == 0).all()
    beg, end, offs = m.get_ranges(pats, 17)
    # a stopped search left characters over and its range is at most 17 rows; never inside the last LOOKUP_LEN chars
    stopped = offs > 0
    assert stopped.any()
    assert ((end - beg)[stopped] <= 17).all() and (offs <= 10).all()


def test_new_symbols_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(ROOT, "include", "kiss_hip.h")).read()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), s
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert s in _lib.EXPORTED_SYMBOLS
    assert "kiss_hip_fmi_view_ex" in text and "kiss_hip_fmi_sizes_ex" in text


def _sizes(n, sa_intv, lookup_len):
    z = _lib.FmiSizesEx()
    rc = _lib.load().kiss_hip_fmi_sizes_ex_for(n, sa_intv, lookup_len, ctypes.byref(z))
    return rc, z


@pytest.mark.parametrize("sa_intv,lookup_len", [(0, 0), (33, 0), (4, 15), (1, 15), (100, 3)])
def test_sizes_ex_rejects_unsupported(sa_intv, lookup_len):
    rc, _ = _sizes(1000, sa_intv, lookup_len)
    assert rc == _lib.KISS_HIP_E_UNSUPPORTED


def test_sizes_ex_null_is_invalid():
    assert _lib.load().kiss_hip_fmi_sizes_ex_for(1000, 4, 0, None) == _lib.KISS_HIP_E_INVALID


@pytest.mark.parametrize("n,sa_intv,lookup_len", [(1000, 4, 0), (1000, 1, 14), (4095, 3, 7), (100_000, 32, 1),
                                                  (999, 8, 10)])
def test_sizes_ex_match_the_layout(n, sa_intv, lookup_len):
    rc, z = _sizes(n, sa_intv, lookup_len)
    assert rc == 0
    N = n + 1
    c = expected_counts(N, sa_intv, lookup_len)
    assert z.base.n_sa == N and z.base.bwt_bytes == (N + 3) // 4
    assert z.base.occ1_entries == c["occ1"] * 4 and z.base.occ2_bytes == c["occ2"] * 4
    assert z.base.sa_entries == c["sa"] and z.lookup_entries == c["lookup"]
    if sa_intv == 1:
        assert z.base.b_words == 0 and z.base.b_occ_entries == 0
    else:
        assert z.base.b_words == (N + 63) // 64 and z.base.b_occ_entries == c["b_occ"]
    if (sa_intv, lookup_len) == (4, 0):  # the original instantiation: exactly kiss_hip_fmi_sizes_for
        old = _lib.FmiSizes()
        assert _lib.load().kiss_hip_fmi_sizes_for(ctypes.c_uint64(n), ctypes.byref(old)) == 0
        assert bytes(old) == bytes(z.base)


def test_ex_structs_match_the_header():
    from tests.test_abi import _sizeof_from_header
    assert ctypes.sizeof(_lib.FmiViewEx) == _sizeof_from_header("kiss_hip_fmi_view_ex")
    assert ctypes.sizeof(_lib.FmiSizesEx) == _sizeof_from_header("kiss_hip_fmi_sizes_ex")


def test_python_parameters_are_checked():
    import kiss_amd.fm_index as fm
    for bad in ({"sa_intv": 0}, {"sa_intv": 33}, {"lookup_len": 15}, {"lookup_len": -1}):
        with pytest.raises(ValueError):
            fm.FMIndex(**bad)
    f = fm.FMIndex()
    assert (f.sa_intv, f.lookup_len) == (4, 0)
