"""GPU tests of FMIndex<SA_INTV>{.LOOKUP_LEN} for SA_INTV in 1..32 and LOOKUP_LEN in 0..14 (kiss_hip_fmi_*_ex_*):
.fmi bytes, the lookup table, get_range with stop_cnt and offsets, and get_offsets, against the numpy model
(tests/fm_model.py) and, at (4, 0), against the C oracle and the original entry points."""
import ctypes
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gen
from tests.fm_model import FmModel
from tests.fmi_layout import canonical

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KISS = os.path.join(ROOT, "kiss_amd", "kiss")
U32 = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def text_and_sa(kind, n, seed):
    from tests import oracle_binding
    if kind == "iid":
        S = gen.iid(n, seed)
    elif kind == "genome":
        S = gen.genome_like(n, seed)
    else:  # "repeats": tandem arrays long enough for the locate walk to reach depth 31 on heavy ranges
        rng = np.random.default_rng(seed)
        S = gen.iid(n, seed)
        S[:n // 8] = np.tile(np.array([0, 1, 2], np.uint8), n // 24 + 1)[:n // 8]
        S[n // 3:n // 3 + n // 10] = 3
        unit = rng.integers(0, 4, 11, dtype=np.uint8)
        S[n // 2:n // 2 + n // 10] = np.tile(unit, n // 110 + 1)[:n // 10]
        S[-200:] = 0  # the text ends inside a repeat: the short suffixes sit in heavy ranges
    SA = oracle_binding.load().suffix_sort(S, 32)
    return S, SA


def patterns_of(S, Q, L, seed, mut=0.15):
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, S.size - L, Q)
    pats = S[pos[:, None] + np.arange(L)[None, :]].copy()
    m = rng.random(Q) < mut
    col = rng.integers(0, L, Q)
    pats[m, col[m]] = (pats[m, col[m]] + 1 + rng.integers(0, 3, int(m.sum()))) % 4
    return np.ascontiguousarray(pats, dtype=np.uint8)


SMALL = [(n, s, l) for n in (1000, 4095) for s in (1, 2, 3, 4, 8, 32) for l in (0, 1, 7, 10)]
DIAGONAL = [(100_000, 1, 10), (100_000, 8, 7), (100_000, 3, 1), (1_000_000, 32, 10), (1_000_000, 2, 1),
            (1_000_000, 1, 0)]


@pytest.mark.parametrize("n,sa_intv,lookup_len", SMALL + DIAGONAL)
def test_fmi_bytes_equal_the_model(n, sa_intv, lookup_len):
    import kiss_amd.fm_index as fm
    S, SA = text_and_sa("iid" if n < 100_000 else "genome", n, 7)
    f = fm.FMIndex(sa_intv=sa_intv, lookup_len=lookup_len).build(S)  # sorts on the GPU with k = 32
    want = FmModel(S, SA, sa_intv, lookup_len).serialize()
    got = f.to_bytes()
    assert got == want
    g = fm.FMIndex.from_bytes(got, sa_intv=sa_intv)  # round trip, L read from the lookup_ count
    assert g.lookup_len == lookup_len and g.to_bytes() == want
    f.close()
    g.close()


def test_full_table_l10_equals_the_model():
    import kiss_amd.fm_index as fm
    S, SA = text_and_sa("repeats", 100_000, 3)
    f = fm.FMIndex(sa_intv=4, lookup_len=10).build(S, sa=SA)
    assert np.array_equal(f.lookup.cpu().numpy().view(np.uint32), FmModel(S, SA, 4, 10).lookup)
    f.close()


def test_table_l14_on_one_million_bases():
    import torch
    import kiss_amd.fm_index as fm
    S, SA = text_and_sa("genome", 1_000_000, 11)
    f = fm.FMIndex(sa_intv=1, lookup_len=14).build(S, sa=SA)
    table = f.lookup.cpu().numpy().view(np.uint32)
    assert table.size == 4 ** 14 + 1 and table[-1] == S.size + 1
    # (a) 2^22 sampled keys against the GPU's own LOOKUP_LEN = 0 backward search of the same 14-mers, without early
    # stop (stop_cnt + 1 wraps to 0): all 14 steps even where the range is empty, as build_lookup does
    plain = fm.FMIndex().build(S, sa=SA)
    keys = np.random.default_rng(1).integers(0, 4 ** 14, 1 << 22)
    shifts = 2 * np.arange(13, -1, -1)
    pats = ((keys[:, None] >> shifts[None, :]) & 3).astype(np.uint8)
    r = plain.query_batch(None, want_offsets=False, d_patterns=torch.from_numpy(pats).cuda(), stop_cnt=U32)
    assert np.array_equal(table[keys], r["beg"])
    r0 = plain.query_batch(None, want_offsets=False, d_patterns=torch.from_numpy(pats).cuda())
    hit = r0["end"] > r0["beg"]
    assert hit.any() and np.array_equal(table[keys][hit], r0["beg"][hit])
    # (b) every key next to a distinct 14-mer of the text and to the A-padded short suffixes, against the model
    m = FmModel(S, SA, 1, 0, with_lookup=False)
    win = np.lib.stride_tricks.sliding_window_view(S.astype(np.int64), 14)
    kmers = np.unique((win << shifts[None, :]).sum(axis=1))
    tail = [int(sum(int(c) << (2 * (13 - i)) for i, c in enumerate(S[S.size - j:]))) for j in range(1, 14)]
    near = np.unique(np.concatenate([kmers, kmers + 1, np.maximum(kmers - 1, 0), tail, np.array(tail) + 1]))
    near = near[near < 4 ** 14]
    beg, _ = m.search_keys(near, 14)
    assert np.array_equal(table[near], beg.astype(np.uint32))
    f.close()
    plain.close()


CONFIGS = [(1, 14), (4, 14), (8, 7), (32, 10), (3, 1), (2, 0), (31, 13), (4, 0)]


@functools.lru_cache(maxsize=None)
def built(sa_intv, lookup_len):
    import kiss_amd.fm_index as fm
    S, SA = text_and_sa("repeats", 300_000, 5)
    return S, fm.FMIndex(sa_intv=sa_intv, lookup_len=lookup_len).build(S, sa=SA), FmModel(S, SA, sa_intv, lookup_len)


@pytest.mark.parametrize("sa_intv,lookup_len", CONFIGS)
@pytest.mark.parametrize("L", [1, 13, 14, 20, 32])
def test_queries_equal_the_model(sa_intv, lookup_len, L):
    S, f, m = built(sa_intv, lookup_len)
    pats = patterns_of(S, 400 if L > 1 else 64, L, 100 + L)
    heavy = np.random.default_rng(L).integers(0, S.size // 8 - L, 40)  # inside the period-3 array: ~10^4 hits each
    pats[:40] = S[heavy[:, None] + np.arange(L)[None, :]]
    pats[40:60] = S[S.size // 2 + np.arange(20)[:, None] + np.arange(L)[None, :]]  # the period-11 array
    pats[60:64] = S[S.size - L - np.arange(4)[:, None] + np.arange(L)[None, :]]    # at the end of the text
    for stop_cnt in (0, 1, 17, U32):
        a = f.query_batch(pats, stop_cnt=stop_cnt, want_offs=True)
        b = m.query_batch(pats, stop_cnt=stop_cnt)
        for k in ("beg", "end", "offs"):
            assert np.array_equal(a[k], b[k]), (k, stop_cnt)
        assert a["total_hits"] == b["total_hits"] and a["checksum"] == b["checksum"], stop_cnt
        assert np.array_equal(a["offsets_index"], b["offsets_index"]), stop_cnt
        assert np.array_equal(a["offsets"], b["offsets"]), stop_cnt


def test_get_range_forms():
    S, f, m = built(4, 14)
    seed = S[1000:1032]
    assert f.get_range(seed) == tuple(int(x[0]) for x in m.get_ranges(seed[None, :])[:2])
    assert f.get_range(seed, stop_cnt=17, with_offset=True) == tuple(int(x[0]) for x in m.get_ranges(seed[None, :], 17))
    short = S[5:9]  # shorter than LOOKUP_LEN: no table
    assert f.get_range(short, with_offset=True) == tuple(int(x[0]) for x in m.get_ranges(short[None, :]))


def test_lookup_14_against_the_oracle_4_0(oracle):
    import kiss_amd.fm_index as fm
    S, SA = text_and_sa("genome", 400_000, 21)
    f = fm.FMIndex(sa_intv=4, lookup_len=14).build(S)
    ref = oracle.fm_build(S, SA)
    m = FmModel(S, SA, 4, 0, with_lookup=False)
    pats = patterns_of(S, 20_000, 32, 8)
    pats[:8] = np.stack([S[i:i + 32] for i in range(8)])
    a = f.query_batch(pats)
    b = ref.query_batch(pats)
    # lookup_[K + 1] = beg(K + 1) is end(K) except where the rows between are text suffixes shorter than 14 characters
    # (keys ending in T next to the end of the text); those patterns are the reference's own, and rare
    keys = (pats[:, 18:].astype(np.int64) << (2 * np.arange(13, -1, -1))[None, :]).sum(axis=1)
    bk, ek = m.search_keys(keys, 14)
    gap = f.lookup.cpu().numpy().view(np.uint32)[keys + 1] != ek
    assert gap.sum() <= 8
    # (an empty range stops the plain search where it empties and the table's after all 14 characters: only the
    # non-empty ranges have one place)
    ok = ~gap & (b["end"] > b["beg"])
    assert ok.sum() > 10_000
    assert np.array_equal(a["beg"][ok], b["beg"][ok]) and np.array_equal(a["end"][ok], b["end"][ok])
    assert np.array_equal((a["end"] - a["beg"])[~gap], (b["end"] - b["beg"])[~gap])
    if not gap.any():
        assert a["total_hits"] == b["total_hits"] and a["checksum"] == b["checksum"]
        assert np.array_equal(a["offsets"], b["offsets"])
    f.close()


def test_4_0_through_the_new_entry_points(oracle):
    import kiss_amd.fm_index as fm
    from kiss_amd import _lib
    S, SA = text_and_sa("repeats", 300_000, 5)
    old = fm.FMIndex().build(S)
    ref = oracle.fm_build(S, SA)
    assert canonical(old.to_bytes()) == canonical(ref.serialize())
    # the host form of the new build at (4, 0)
    n = S.size
    z = _lib.FmiSizesEx()
    lib = _lib.load()
    assert lib.kiss_hip_fmi_sizes_ex_for(n, 4, 0, ctypes.byref(z)) == 0
    bwt = np.zeros(z.base.bwt_bytes, np.uint8)
    occ1 = np.zeros(z.base.occ1_entries, np.uint32)
    occ2 = np.zeros(z.base.occ2_bytes, np.uint8)
    sa = np.zeros(z.base.sa_entries, np.uint32)
    b = np.zeros(z.base.b_words, np.uint64)
    bocc = np.zeros(z.base.b_occ_entries, np.uint32)
    lookup = np.zeros(z.lookup_entries, np.uint32)
    cnt = (ctypes.c_uint32 * 4)()
    pri = ctypes.c_uint32()
    Sc = np.ascontiguousarray(S)
    assert lib.kiss_hip_fmi_build_ex_host(Sc.ctypes.data, n, None, 4, 0, bwt.ctypes.data, occ1.ctypes.data, occ2.ctypes.data,
                                          sa.ctypes.data, b.ctypes.data, bocc.ctypes.data, lookup.ctypes.data,
                                          ctypes.addressof(cnt), ctypes.addressof(pri), 0) == 0
    assert list(cnt) == old.cnt.tolist() and pri.value == old.pri and lookup.tolist() == [0, n + 1]
    assert np.array_equal(sa, old.sa.cpu().numpy().view(np.uint32))
    assert np.array_equal(b, old.b.cpu().numpy().view(np.uint64)[:b.size])
    assert np.array_equal(bwt, old.bwt.cpu().numpy()[:bwt.size])
    # the query through kiss_hip_fmi_query_ex_dev (want_offs forces it) against the original one
    pats = patterns_of(S, 5000, 24, 2)
    pats[:30] = S[np.arange(30)[:, None] * 97 + np.arange(24)[None, :]]
    a = old.query_batch(pats)
    e = old.query_batch(pats, want_offs=True)
    for k in ("beg", "end", "offsets", "offsets_index"):
        assert np.array_equal(a[k], e[k]), k
    assert a["total_hits"] == e["total_hits"] and a["checksum"] == e["checksum"]
    hit = e["end"] > e["beg"]  # stop_cnt = 0 stops only on an empty range, which leaves characters unmatched
    assert (e["offs"][hit] == 0).all() and (e["offs"][~hit] > 0).any()
    old.close()


@pytest.mark.parametrize("sa_intv", (1, 4))
def test_host_entries_build_and_query_equal_the_model(sa_intv):
    """kiss_hip_fmi_build_ex_host (sorting itself, and from a suffix array) and kiss_hip_fmi_query_ex_host on its arrays, with and
    without the sampling bit-vector: the empty batch, the call without any optional output, the call with all of them"""
    from kiss_amd import _lib
    lib = _lib.load()
    n, lookup_len, L, Q = 4095, 3, 7, 64
    S, SA = text_and_sa("iid", n, 7)
    m = FmModel(S, SA, sa_intv, lookup_len)
    z = _lib.FmiSizesEx()
    assert lib.kiss_hip_fmi_sizes_ex_for(n, sa_intv, lookup_len, ctypes.byref(z)) == 0
    Sc, SAc = np.ascontiguousarray(S), np.ascontiguousarray(SA, np.uint32)
    assert SAc.size == n + 1

    def build(sa):
        a = {"bwt": np.zeros(z.base.bwt_bytes, np.uint8), "occ1": np.zeros(z.base.occ1_entries, np.uint32),
             "occ2": np.zeros(z.base.occ2_bytes, np.uint8), "sa": np.zeros(z.base.sa_entries, np.uint32),
             "b": np.zeros(z.base.b_words, np.uint64), "b_occ": np.zeros(z.base.b_occ_entries, np.uint32),
             "lookup": np.zeros(z.lookup_entries, np.uint32)}
        cnt, pri = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
        p = {k: x.ctypes.data if x.size else None for k, x in a.items()}  # (sa_intv == 1: no b / b_occ)
        assert lib.kiss_hip_fmi_build_ex_host(Sc.ctypes.data, n, sa.ctypes.data if sa is not None else None, sa_intv, lookup_len, p["bwt"],
                                              p["occ1"], p["occ2"], p["sa"], p["b"], p["b_occ"], p["lookup"], ctypes.addressof(cnt),
                                              ctypes.addressof(pri), 0) == 0
        return a, list(cnt), pri.value

    a, cnt, pri = build(None)
    a2, cnt2, pri2 = build(SAc)
    assert (cnt, pri) == (cnt2, pri2) and all(np.array_equal(a[k], a2[k]) for k in a)
    import kiss_amd.fm_index as fm
    f = fm.FMIndex(sa_intv=sa_intv, lookup_len=lookup_len).build(S, sa=SA)  # the device entry (its bytes: test_fmi_bytes_equal_the_model)
    assert cnt == f.cnt.tolist() and pri == f.pri
    for k, x in a.items():
        assert np.array_equal(x, getattr(f, k).cpu().numpy().view(x.dtype)[:x.size]) if x.size else getattr(f, k) is None, k
    f.close()
    v = _lib.FmiViewEx()
    v.base.n_sa, v.base.pri, v.base.sa_intv, v.lookup_len, v.lookup = n + 1, pri, sa_intv, lookup_len, a["lookup"].ctypes.data
    for c in range(4):
        v.base.cnt[c] = cnt[c]
    for k in ("bwt", "occ1", "occ2", "sa", "b", "b_occ"):
        setattr(v.base, k, a[k].ctypes.data if a[k].size else None)
    pats = patterns_of(S, Q, L, 3, mut=0.3)
    want = m.query_batch(pats, stop_cnt=0)
    hits = (want["end"] - want["beg"]).astype(np.int64)
    assert (hits == 0).any() and (hits > 1).any()

    def query(Q, optional, cap):
        beg, end, offs = np.full(Q + 1, 7, np.uint32), np.full(Q + 1, 7, np.uint32), np.full(Q + 1, 7, np.uint32)
        offsets, oidx = np.zeros(max(cap, 1), np.uint32), np.full(Q + 1, 7, np.uint64)
        tot, chk = ctypes.c_uint64(99), ctypes.c_uint64(99)
        rc = lib.kiss_hip_fmi_query_ex_host(ctypes.byref(v), pats.ctypes.data if Q else None, L, Q, 0, beg.ctypes.data, end.ctypes.data,
                                            offs.ctypes.data if optional else None, ctypes.byref(tot) if optional else None,
                                            ctypes.byref(chk) if optional else None, offsets.ctypes.data if optional else None,
                                            oidx.ctypes.data if optional else None, cap if optional else 0, 0)
        return rc, beg[:Q], end[:Q], offs[:Q], tot.value, chk.value, offsets[:cap], oidx

    rc, beg, end, offs, tot, chk, offsets, oidx = query(0, True, 0)  # the empty batch
    assert rc == 0 and (tot, chk) == (0, 0)
    rc, beg, end, offs, tot, chk, offsets, oidx = query(Q, False, 0)
    assert rc == 0 and np.array_equal(beg, want["beg"]) and np.array_equal(end, want["end"]) and (tot, chk) == (99, 99)
    rc, beg, end, offs, tot, chk, offsets, oidx = query(Q, True, want["total_hits"])
    assert rc == 0 and np.array_equal(beg, want["beg"]) and np.array_equal(end, want["end"]) and np.array_equal(offs, want["offs"])
    assert (tot, chk) == (want["total_hits"], want["checksum"])
    assert np.array_equal(oidx, want["offsets_index"]) and np.array_equal(offsets, want["offsets"])


def test_from_bytes_rejects_a_mismatched_file():
    import kiss_amd.fm_index as fm
    S, f, _ = built(1, 14)
    buf = f.to_bytes()
    for wrong in (4, 2, 32):
        with pytest.raises(ValueError):
            fm.FMIndex.from_bytes(buf, sa_intv=wrong)
    S4, f4, _ = built(4, 0)
    buf4 = f4.to_bytes()
    with pytest.raises(ValueError):
        fm.FMIndex.from_bytes(buf4, sa_intv=8)
    # a lookup_ whose count is not 4^L + 1
    bad = bytearray(buf)
    sa_count_off = 20 + 8 + (f.N + 3) // 4
    sa_count_off += 8 + f.occ1.numel() * 4
    sa_count_off += 8 + f.occ2.numel()
    sa_count_off += 8 + f.sa.numel() * 4  # -> the lookup_ count
    struct.pack_into("<Q", bad, sa_count_off, 4 ** 14)
    with pytest.raises(ValueError):
        fm.FMIndex.from_bytes(bytes(bad), sa_intv=1)


def write_text(path, S):
    with open(path, "w") as f:
        f.write(">t\n")
        s = "".join("ACGT"[c] for c in S)
        for i in range(0, len(s), 80):
            f.write(s[i:i + 80] + "\n")


def test_cli_round_trip(tmp_path):
    S, SA = text_and_sa("repeats", 300_000, 5)
    fa = str(tmp_path / "r.fa")
    write_text(fa, S)
    r = subprocess.run([KISS, "fmindex_build", fa, "--sa-intv", "1", "--lookup-len", "8"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    m = FmModel(S, SA, 1, 8)
    assert open(fa + ".fmi", "rb").read() == m.serialize()
    q = S[1000:1024]
    qs = "".join("ACGT"[c] for c in q)
    r = subprocess.run([KISS, "fmindex_query", fa, "--sa-intv", "1", "-q", qs, "-n", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = m.query_batch(q[None, :])
    assert "query = %s found %d times" % (qs, want["total_hits"]) in r.stderr
    assert "The 1-st position is %d, content of substring is %s" % (int(want["offsets"][0]), qs) in r.stderr
    Q, L = 3000, 32
    pats = patterns_of(S, Q, L, 6)
    pf = str(tmp_path / "patterns.bin")
    with open(pf, "wb") as f:
        f.write(struct.pack("<II", L, Q))
        f.write(bytes(ord("ACGT"[c]) for c in pats.reshape(-1)))
    r = subprocess.run([KISS, "fmindex_query", fa, "--sa-intv", "1", "-b", pf], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    want = m.query_batch(pats, want_offsets=False)
    assert "number of matched locations: %d" % want["total_hits"] in r.stderr
    assert "location checksum: %d" % want["checksum"] in r.stderr
    # the file does not record SA_INTV: the wrong one is an error, not a wrong answer
    r = subprocess.run([KISS, "fmindex_query", fa, "-b", pf], capture_output=True, text=True)
    assert r.returncode != 0 and "sa-intv" in r.stderr
    r = subprocess.run([KISS, "fmindex_query", fa, "--sa-intv", "8", "-q", qs], capture_output=True, text=True)
    assert r.returncode != 0
