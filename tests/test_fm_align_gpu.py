"""kiss_hip_fmi_align_dev / _host against tests/fm_align_model.py, element by element: (a) synthetic chain records through
kiss_amd.align_chains, (b) the error contract of the raw device call, (c) FMIndex.align on the texts of the FM tests, the
alignments compared with the model run on the chains the device returned."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm_align_model as am
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu

PARAM_SETS = (dict(match=1, mismatch=4, gap_open=6, gap_extend=1), dict(match=2, mismatch=3, gap_open=0, gap_extend=1),
              dict(match=1, mismatch=1, gap_open=1, gap_extend=0), dict(match=3, mismatch=0, gap_open=0, gap_extend=0))
REPORT_KEYS = ("aligned", "too_wide", "cells", "best_score", "max_band")


def check(res, want, cigar=True, key="report"):
    got = np.stack([res["alignments"][k].astype(np.int64) for k in am.FIELDS], axis=1).reshape(-1, 12)
    assert got.shape == want["alignments"].shape
    for c in np.flatnonzero((got != want["alignments"]).any(axis=1))[:3]:
        raise AssertionError("alignment %d: %s, the model says %s" % (c, dict(zip(am.FIELDS, got[c])), dict(zip(am.FIELDS, want["alignments"][c]))))
    rep = res[key]
    assert rep["chains"] == got.shape[0] and rep["cigar_ops"] == want["cigar"].size
    assert {k: rep[k] for k in REPORT_KEYS} == {k: want[k] for k in REPORT_KEYS}
    if cigar:
        assert np.array_equal(res["cigar_index"], want["cigar_index"])
        assert np.array_equal(res["cigar"], want["cigar"])


def run(S, reads, quads, cidx, both=False, **params):
    import kiss_amd
    want = am.align(S, reads, quads, cidx, both, **params)
    res = kiss_amd.align_chains(S, reads, np.asarray(quads, np.int64).reshape(-1, 4), cidx, both_strands=both, **params)
    check(res, want)
    return want


def mutate(piece, rng, subs=2, indels=2):
    """a piece of text with substitutions and 1..3-base insertions and deletions"""
    R = np.asarray(piece, np.uint8).copy()
    for _ in range(subs):
        if R.size:
            j = int(rng.integers(0, R.size))
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
    for _ in range(indels):
        if R.size > 8:
            j, g = int(rng.integers(4, R.size - 4)), int(rng.integers(1, 4))
            R = np.concatenate([R[:j], rng.integers(0, 4, g, dtype=np.uint8), R[j:]]) if rng.random() < 0.5 else np.concatenate([R[:j], R[j + g:]])
    return R


@functools.lru_cache(maxsize=None)
def random_text(n=2000, seed=11):
    return np.random.default_rng(seed).integers(0, 4, n, dtype=np.uint8)


# band and d1 - d0 that give B = 1, 63, 64, 65, 129, 1024, 1025 (the last one is too wide)
BANDS = ((0, 0), (31, 0), (31, 1), (32, 0), (64, 0), (511, 1), (512, 0))


@pytest.mark.parametrize("band,skew", BANDS)
def test_read_lengths_under_every_band_width(band, skew):
    S = random_text()
    rng = np.random.default_rng(band + skew)
    reads, quads, cidx = [], [], [0]
    for L in (1, 2, 63, 64, 65, 150, 300):
        for p in (0, 700, S.size - L):  # windows clipped at both ends of the text, and one inside
            R = mutate(S[p:p + L], rng, subs=L // 50, indels=L // 60)[:L]
            if R.size < L:
                R = np.concatenate([R, rng.integers(0, 4, L - R.size, dtype=np.uint8)])
            reads.append(R)
            quads.append((0, L, p, p + L + skew))
            cidx.append(len(quads))
    want = run(S, reads, quads, cidx, band=band)
    B = 2 * band + skew + 1
    assert (want["alignments"][:, 11] == B).all()
    if B > am.MAX_BAND:
        assert want["too_wide"] == len(quads) and want["cells"] == 0 and (want["alignments"][:, 1] == am.BAND_TOO_WIDE).all()
        assert not want["alignments"][:, (0, 2, 3, 4, 5, 6, 7, 8, 9, 10)].any() and want["cigar"].size == 0
    else:
        assert want["too_wide"] == 0 and (want["alignments"][:, 0] > 0).all()
        assert band < 31 or (want["alignments"][:, 10] > 0).any()  # (gaps where the band leaves room for them)


def test_the_pins():
    import kiss_amd
    S = np.random.default_rng(11).integers(0, 4, 400).astype(np.uint8)
    n = S.size
    rng = np.random.default_rng(4)
    exact = S[100:250].copy()
    sub = exact.copy()
    sub[75] = (sub[75] + 1) & 3
    cut = np.concatenate([S[100:175], S[178:253]])
    front = np.concatenate([(S[:5][::-1] + 1) & 3, S[:145]])
    back = np.concatenate([S[n - 143:], rng.integers(0, 4, 7, dtype=np.uint8)])

    def one(R, quad, **params):
        res = kiss_amd.align_chains(S, [R], [quad], [0, 1], **params)
        check(res, am.align(S, [R], [quad], [0, 1], **params))
        return {k: int(res["alignments"][k][0]) for k in am.FIELDS}, am.cigar_string([(int(o) & 15, int(o) >> 4) for o in res["cigar"]])

    rec, cigar = one(exact, (0, 150, 100, 250))
    assert (rec["score"], cigar, rec["band"]) == (150, "150M", 65)
    rec, cigar = one(sub, (0, 150, 100, 250))
    assert (rec["score"], cigar, rec["rbeg"], rec["rend"]) == (145, "150M", 0, 150)
    rec, cigar = one(cut, (0, 150, 100, 250), band=3)
    assert (rec["score"], rec["tend"] - rec["tbeg"], rec["band"], cigar) == (141, 153, 7, "75M3D75M")
    rec, cigar = one(cut, (0, 150, 100, 250), band=2)
    assert (rec["score"], rec["rend"], rec["band"]) == (75, 75, 5)
    rec, cigar = one(cut, (0, 150, 100, 253), band=0)
    assert (rec["score"], rec["band"]) == (141, 4)
    rec, cigar = one(front, (5, 150, 0, 145))
    assert (rec["rbeg"], rec["tbeg"], rec["score"]) == (5, 0, 145)
    rec, cigar = one(back, (0, 143, n - 143, n))
    assert (rec["tend"], rec["rend"], rec["score"]) == (n, 143, 143)
    g = np.random.default_rng(3)
    X, Y = g.integers(1, 4, 20, dtype=np.uint8), g.integers(1, 4, 20, dtype=np.uint8)
    S2, R2 = np.concatenate([X, np.zeros(8, np.uint8), Y]), np.concatenate([X, np.zeros(6, np.uint8), Y])
    res = kiss_amd.align_chains(S2, [R2], [(0, 46, 0, 48)], [0, 1])
    check(res, am.align(S2, [R2], [(0, 46, 0, 48)], [0, 1]))
    assert am.cigar_string([(int(o) & 15, int(o) >> 4) for o in res["cigar"]]) == "20M2D26M"


def test_negative_diagonals_clipped_windows_and_bands_outside_the_text():
    S = random_text()
    n = S.size
    rng = np.random.default_rng(8)
    R = mutate(S[0:140], rng)
    reads = [np.concatenate([rng.integers(0, 4, 60, dtype=np.uint8), R]),  # 60 bases in front of the text: d = -60
             np.concatenate([mutate(S[n - 120:], rng), rng.integers(0, 4, 80, dtype=np.uint8)]),  # 80 behind it
             S[500:650].copy()]
    quads = [(60, 200, 0, 140), (0, 120, n - 120, n),
             (0, 150, n + 5000, n + 5150),  # the whole band behind the text
             (3000, 3150, 0, 150),          # the whole band in front of it
             (0, 150, n - 10, n + 140),     # ten columns of it inside
             (140, 150, 0, 10),             # ten rows of it inside
             (0, 150, 500, 650)]
    want = run(S, reads, quads, [0, 1, 2, 7], band=20)
    assert list(want["alignments"][2:4, 0]) == [0, 0] and want["alignments"][6, 0] == 150 and want["alignments"][0, 2] >= 60
    assert want["aligned"] == 7 and want["cells"] == (reads[0].size + reads[1].size + 5 * 150) * 41


def test_no_bases():
    S = random_text()
    rng = np.random.default_rng(9)
    alln = np.full(70, 78, np.uint8)
    some = S[300:500].copy()
    some[rng.integers(0, 200, 12)] = 78
    one = S[900:965].copy()
    one[0] = one[64] = 4
    want = run(S, [alln, some, one, np.array([255], np.uint8)], [(0, 70, 100, 170), (0, 200, 300, 500), (0, 65, 900, 965), (0, 1, 5, 6)],
               [0, 1, 2, 3, 4])
    assert want["alignments"][0, 0] == 0 and want["alignments"][3, 0] == 0 and want["alignments"][1, 7] >= 1
    want = run(S, [some], [(0, 200, 300, 500)], [0, 1], match=5, mismatch=1, gap_open=2, gap_extend=2, band=4)
    assert want["alignments"][0, 7] >= 10  # (a no-base column costs 1: cheaper than the ends it joins)


def revcomp(R):
    return am.virtual_read(R, True)


def test_odd_virtual_reads_are_reverse_complements():
    S = random_text()
    rng = np.random.default_rng(10)
    fwd = mutate(S[100:250], rng)
    rev = revcomp(mutate(S[1200:1400], rng))  # its reverse complement lies in the text
    rev[17] = 78
    mid = S[600:601].copy()
    reads = [fwd, rev, mid, revcomp(S[1700:1765])]
    # virtual reads 0..7: chains on 0, 3 (two), 4, 5, 7; none on 1, 2, 6
    quads = [(0, fwd.size, 100, 250), (0, rev.size, 1200, 1400), (10, 60, 1210, 1262), (0, 1, 600, 601), (0, 1, 600, 601), (0, 65, 1700, 1765)]
    want = run(S, reads, quads, [0, 1, 1, 1, 3, 4, 5, 5, 6], both=True, band=10)
    assert want["alignments"][1, 0] > 150 and want["alignments"][3, 0] == 1 and want["alignments"][5, 0] == 65


@pytest.mark.parametrize("kind", ("AC", "A"))
def test_texts_full_of_ties(kind):
    S = np.tile(np.array([0, 1], np.uint8), 600) if kind == "AC" else np.zeros(1200, np.uint8)
    reads = [S[:90].copy(), S[1:66].copy(), np.concatenate([S[:40], [3, 3], S[:41]]).astype(np.uint8), S[:64].copy()]
    quads = [(0, 90, 300, 390), (0, 65, 1, 66), (0, 83, 500, 583), (0, 64, S.size - 40, S.size + 24), (0, 64, 0, 70)]
    for p in (PARAM_SETS[0], PARAM_SETS[3]):
        run(S, reads, quads, [0, 1, 2, 3, 5], **p, band=33)


@pytest.mark.parametrize("which", range(len(PARAM_SETS) + 1))
def test_parameter_sets(which):
    S = random_text()
    rng = np.random.default_rng(20 + which)
    p = PARAM_SETS[which] if which < len(PARAM_SETS) else dict(match=65535, mismatch=65535, gap_open=65535, gap_extend=65535)
    reads, quads, cidx = [], [], [0]
    for L, at in ((150, 100), (300, 900), (64, 1500), (31, 40)):
        reads.append(mutate(S[at:at + L], rng, subs=3, indels=3))
        quads.append((0, reads[-1].size, at, at + L))
        cidx.append(len(quads))
    want = run(S, reads, quads, cidx, **p, band=12)
    assert (want["alignments"][:, 0] > 0).all()
    if which == len(PARAM_SETS):
        assert want["best_score"] > 65535 * 40


def test_reads_without_chains_an_offset_index_and_empty_batches():
    import kiss_amd
    S = random_text()
    rng = np.random.default_rng(12)
    reads = [mutate(S[at:at + 100], rng) for at in (0, 200, 400, 600, 800)]
    unused = [(1, 2, 3, 4)] * 3  # chains in front of chain_index[0]: not this call's
    quads = unused + [(0, 100, 200, 300), (5, 90, 205, 290), (0, 100, 1000, 1100), (0, 100, 800, 900)]
    want = run(S, reads, quads, [3, 3, 6, 6, 6, 7])
    assert want["alignments"].shape[0] == 4 and want["alignments"][3, 0] > 50
    res = kiss_amd.align_chains(S, reads, np.asarray(quads, np.int64), [3, 3, 6, 6, 6, 7], want_cigar=False)  # the records alone
    assert "cigar" not in res and "cigar_index" not in res
    check(res, want, cigar=False)
    # no chains at all, and no reads at all
    res = kiss_amd.align_chains(S, reads, np.zeros((0, 4), np.int64), [0] * 6)
    assert res["alignments"].shape == (0,) and list(res["cigar_index"]) == [0] and res["report"]["chains"] == 0
    res = kiss_amd.align_chains(S, reads, unused, [3] * 6)
    assert res["alignments"].shape == (0,) and list(res["cigar_index"]) == [0]
    res = kiss_amd.align_chains(S, [], np.zeros((0, 4), np.int64), [0], both_strands=True)
    assert res["alignments"].shape == (0,) and list(res["cigar_index"]) == [0] and res["report"]["V"] == 0


def test_a_one_base_read_beside_one_of_3000_bases_at_the_widest_band():
    S = random_text()
    rng = np.random.default_rng(13)
    long = np.concatenate([mutate(S[:1500], rng, subs=30, indels=20), rng.integers(0, 4, 1600, dtype=np.uint8)])[:3000]
    reads = [S[77:78].copy(), long, S[1999:2000].copy()]
    want = run(S, reads, [(0, 1, 77, 78), (0, 3000, 0, 3001), (0, 1, 1999, 2000)], [0, 1, 2, 3], band=511)
    assert want["max_band"] == 1024 and want["cells"] == 1024 * 3000 + 2 * 1023 and want["alignments"][1, 0] > 1000
    assert list(want["alignments"][(0, 2), 0]) == [1, 1]


# ---- (b) the error contract of the C call ------------------------------------------------------------------------------------
def raw_dev(S, reads, quads, cidx, aln_capacity, cigar_capacity=None, both=False, max_n=1 << 20, params=None, **kw):
    """kiss_hip_fmi_align_dev itself -> rc, report, alns (n x 12), cigar, cigar_index"""
    import torch
    import kiss_amd
    from kiss_amd import _lib, fm_align
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    vp = ctypes.c_void_p
    cat = np.concatenate(reads).astype(np.uint8)
    ridx = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([r.size for r in reads], out=ridx[1:])
    ch = np.zeros((max(len(quads), 1), 6), np.int64)
    ch[:len(quads), 2:6] = np.asarray(quads, np.int64).reshape(-1, 4)
    d_text = torch.from_numpy(np.asarray(S, np.uint8)).to(dev)
    d_reads, d_ridx = torch.from_numpy(cat).to(dev), torch.from_numpy(ridx).to(dev)
    d_chains = torch.from_numpy(ch.astype(np.uint32).view(np.int32)).to(dev)
    d_cidx = torch.from_numpy(np.asarray(cidx, np.int64)).to(dev)
    C = max(int(cidx[-1]) - int(cidx[0]), 0)
    d_alns = torch.full((max(aln_capacity, 1), 12), -1, dtype=torch.int32, device=dev)
    d_cig = d_oidx = None
    if cigar_capacity is not None:
        d_cig = torch.full((max(cigar_capacity, 1),), -1, dtype=torch.int32, device=dev)
        d_oidx = torch.full((C + 1,), -1, dtype=torch.int64, device=dev)
    rep = _lib.AlignReport()
    p = params if params is not None else fm_align.align_params(**kw)
    with kiss_amd.Context(max_n=max_n) as ctx:
        rc = lib.kiss_hip_fmi_align_dev(ctx._ctx, vp(d_text.data_ptr()), int(np.asarray(S).size), vp(d_reads.data_ptr()),
                                        vp(d_ridx.data_ptr()), len(reads), 1 if both else 0, vp(d_chains.data_ptr()),
                                        vp(d_cidx.data_ptr()), ctypes.byref(p), vp(d_alns.data_ptr()), aln_capacity,
                                        vp(d_cig.data_ptr()) if d_cig is not None else None,
                                        vp(d_oidx.data_ptr()) if d_oidx is not None else None, cigar_capacity or 0,
                                        ctypes.byref(rep), None)
    return (rc, rep, d_alns.cpu().numpy(), d_cig.cpu().numpy() if d_cig is not None else None,
            d_oidx.cpu().numpy() if d_oidx is not None else None)


def test_error_contract_of_the_c_call():
    import kiss_amd
    from kiss_amd import _lib
    S = random_text()
    rng = np.random.default_rng(14)
    reads = [mutate(S[at:at + 120], rng) for at in (0, 300, 600, 900)]
    quads = [(0, 120, at, at + 120) for at in (0, 300, 305, 600, 900)]
    cidx = [0, 1, 3, 4, 5]
    params = dict(band=9)
    want = am.align(S, reads, quads, cidx, **params)
    C, m = 5, int(want["cigar"].size)
    assert m > C
    # capacities one short: E_INVALID with the totals in the report, and nothing written
    rc, rep, alns, cig, oidx = raw_dev(S, reads, quads, cidx, C - 1, m, **params)
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.chains, rep.cigar_ops, rep.cells) == (C, m, want["cells"])
    assert (alns == -1).all() and (cig == -1).all() and (oidx == -1).all()
    rc, rep, alns, cig, oidx = raw_dev(S, reads, quads, cidx, C, m - 1, **params)
    assert rc == _lib.KISS_HIP_E_INVALID and (rep.chains, rep.cigar_ops) == (C, m)
    assert (alns == -1).all() and (cig == -1).all() and (oidx == -1).all()
    # with room, and without the ops
    rc, rep, alns, cig, oidx = raw_dev(S, reads, quads, cidx, C, m, **params)
    assert rc == 0 and np.array_equal(alns.view(np.uint32).astype(np.int64), want["alignments"])
    assert np.array_equal(cig.view(np.uint32), want["cigar"]) and np.array_equal(oidx.astype(np.uint64), want["cigar_index"])
    assert rep.best_score == want["best_score"] and rep.max_band == 19 and rep.ms_total > 0 and rep.ms_dp > 0
    rc, rep, alns, cig, oidx = raw_dev(S, reads, quads, cidx, C, None, **params)
    assert rc == 0 and cig is None and np.array_equal(alns.view(np.uint32).astype(np.int64), want["alignments"])
    assert rep.cigar_ops == m
    # a chain_index that decreases, a read of length 0
    assert raw_dev(S, reads, quads, [0, 1, 3, 2, 5], C, m, **params)[0] == _lib.KISS_HIP_E_INVALID
    assert raw_dev(S, reads[:2] + [np.zeros(0, np.uint8)] + reads[2:], quads, cidx + [5], C, m, **params)[0] == _lib.KISS_HIP_E_INVALID
    with pytest.raises(kiss_amd.KissHipError) as e:
        kiss_amd.align_chains(S, reads, quads, [0, 1, 3, 2, 5], **params)
    assert e.value.status == _lib.KISS_HIP_E_INVALID
    # parameters out of range, cigar without cigar_index
    lib = _lib.load()
    buf = np.zeros(64, np.uint64)
    b = buf.ctypes.data
    for p in (_lib.AlignParams(match=0, mismatch=4, gap_open=6, gap_extend=1, band=32), _lib.AlignParams(match=65536),
              _lib.AlignParams(match=1, mismatch=65536), _lib.AlignParams(match=1, gap_open=65536),
              _lib.AlignParams(match=1, gap_extend=65536), _lib.AlignParams(match=1, band=1 << 31)):
        assert lib.kiss_hip_fmi_align_host(b, 8, b, b, 1, 0, b, b, ctypes.byref(p), b, 1, None, None, 0, None, 0) == _lib.KISS_HIP_E_INVALID
        assert raw_dev(S, reads, quads, cidx, C, m, params=p)[0] == _lib.KISS_HIP_E_INVALID
    p = _lib.AlignParams(match=1)
    assert lib.kiss_hip_fmi_align_host(b, 8, b, b, 1, 0, b, b, ctypes.byref(p), b, 1, b, None, 0, None, 0) == _lib.KISS_HIP_E_INVALID
    assert lib.kiss_hip_fmi_align_host(None, 8, b, b, 1, 0, b, b, ctypes.byref(p), b, 1, None, None, 0, None, 0) == _lib.KISS_HIP_E_INVALID


def test_a_batch_just_over_the_cell_limit_of_a_small_context():
    from kiss_amd import _lib
    S = random_text()
    limit = am.CELLS_PER_N << 20
    # five chains of 3000 x 1024 cells, and a gapless one (B = 1) whose read makes the total limit + 1
    rest = limit - 5 * 3000 * 1024 + 1
    reads = [np.zeros(3000, np.uint8), np.zeros(rest, np.uint8)]
    quads = [(0, 3000, 0, 4023)] * 5 + [(0, 10, 0, 10)]
    rc, rep, alns, cig, oidx = raw_dev(S, reads, quads, [0, 5, 6], 6, 100, band=0)
    assert rc == _lib.KISS_HIP_E_UNSUPPORTED and rep.cells == limit + 1 and (rep.chains, rep.aligned) == (6, 6)
    assert (alns == -1).all() and (cig == -1).all()
    # L * match at 2^30
    rc = raw_dev(S, [np.zeros(1 << 14, np.uint8)], [(0, 10, 0, 10)], [0, 1], 1, 100, match=65535, mismatch=1, band=0)[0]
    assert rc == _lib.KISS_HIP_OK
    rc = raw_dev(S, [np.zeros((1 << 14) + 1, np.uint8)], [(0, 10, 0, 10)], [0, 1], 1, 100, match=65535, mismatch=1, band=0)[0]
    assert rc == _lib.KISS_HIP_E_UNSUPPORTED


# ---- (c) FMIndex.align on the texts ------------------------------------------------------------------------------------------
ALIGN_SETS = (dict(), dict(match=2, mismatch=3, gap_open=4, gap_extend=2, band=12))


@functools.lru_cache(maxsize=None)
def reads_of(name):
    """reads cut from the text with substitutions and 1..3-base indels, one random read, one with a no-base"""
    S = text(name)
    n = S.size
    rng = np.random.default_rng(31)
    out = []
    for L in (40, 100, 150, 257):
        if n >= L:
            p = int(rng.integers(0, n - L + 1))
            out.append(mutate(S[p:p + L], rng, subs=max(1, L // 50), indels=max(1, L // 80)))
            q = mutate(S[p:p + L], rng, subs=1, indels=1)
            q[q.size // 3] = 78
            out.append(q)
        else:
            out.append(rng.integers(0, 4, L, dtype=np.uint8))
    out.append(rng.integers(0, 4, 90, dtype=np.uint8))
    return out


@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_alignments_of_reads_equal_the_model_on_the_chains_of_the_device(name, both):
    from tests.test_fm_chain_gpu import index_of
    f = index_of(name, 4)
    S = text(name)
    reads = reads_of(name)
    for which, params in enumerate(ALIGN_SETS):
        res = f.align(reads, S, 15, 0, 200, both_strands=both, chain_params=dict(min_score=25, band=100), **params)
        want = am.align(S, reads, res["chains"], res["chain_index"], both, **params)
        check(res, want, key="align_report")
        assert res["report"]["chains"] == res["alignments"].shape[0]
        if which == 0:  # a device tensor for the text, and no ops
            import torch
            res2 = f.align(reads, torch.from_numpy(S).to("cuda:0") if S.size else S, 15, 0, 200, both_strands=both,
                           chain_params=dict(min_score=25, band=100), want_cigar=False, **params)
            assert "cigar" not in res2 and "cigar_index" not in res2
            check(res2, want, cigar=False, key="align_report")
    if name in ("genome", "iid"):
        assert (res["alignments"]["score"] > 60).sum() >= 4 and (res["alignments"]["gaps"] > 0).any()
