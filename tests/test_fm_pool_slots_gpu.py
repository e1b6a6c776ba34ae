"""The pooled scratch of the FM-index calls (kiss_amd/csrc/kiss_internal.hpp: FmSlot) across calls on ONE context: every kind
of call after every other one, forwards and backwards, and once more after the pool has been regrown.  A slot that two roles
share by mistake, or a buffer that one call leaves in a state the next one trips over, shows as a result that depends on what
ran before; every result is also held against the matching _host entry, which runs on a context of its own.  The other FM
tests mostly make one kind of call per context."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, REPEAT, Q, L = 4096, 200, 64, 48
CALLS = ("query_batch", "query_mismatch", "seeds", "chains", "align", "map")


def _inputs():
    rng = np.random.default_rng(20240611)
    text = rng.integers(0, 4, N).astype(np.uint8)
    text[3000:3000 + REPEAT] = text[500:500 + REPEAT]  # the planted repeat: reads from it have two loci

    def cut(count, seed):
        r = np.random.default_rng(seed)
        starts = r.integers(0, N - L, count)
        starts[:8] = 500 + 19 * np.arange(8)  # (inside the repeat)
        pats = np.stack([text[s:s + L] for s in starts])
        for q in range(1, count, 2):  # every other read: one substitution
            at = int(r.integers(19, L - 19))  # (a seed of min_len on either side)
            pats[q, at] = (pats[q, at] + 1 + int(r.integers(0, 3))) & 3
        return pats

    pats = cut(Q, 1)
    return text, pats, np.concatenate([pats, cut(3 * Q, 2)])


def _run(f, name, text, pats):
    reads = list(pats)
    if name == "query_batch":
        return f.query_batch(pats)
    if name == "query_mismatch":
        return f.query_mismatch(pats, 2)
    if name == "seeds":
        return f.seeds(reads, both_strands=True)
    if name == "chains":
        return f.chains(reads, both_strands=True, want_anchors=True)
    if name == "align":
        return f.align(reads, text, both_strands=True)
    return f.map(reads, text, both_strands=True)


def _same(a, b, where):
    """two results of one call, array for array; of a report everything but its times"""
    assert sorted(a) == sorted(b), where
    for k, x in a.items():
        y = b[k]
        if isinstance(x, dict):
            assert {j: v for j, v in x.items() if not j.startswith("ms_")} == {j: v for j, v in y.items() if not j.startswith("ms_")}, (where, k)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (where, k)
        else:
            assert x == y, (where, k)


@pytest.fixture(scope="module")
def passes():
    import kiss_amd.fm_index as fm
    text, pats, more = _inputs()
    f = fm.FMIndex(sa_intv=4).build(text, exact=True)
    first = {name: _run(f, name, text, pats) for name in CALLS}
    second = {name: _run(f, name, text, pats) for name in reversed(CALLS)}
    regrown = _run(f, "query_batch", text, more)  # 4 x as many patterns: the per-pattern buffers are regrown
    host_index = {k: getattr(f, k).cpu().numpy() for k in ("bwt", "occ1", "occ2", "sa", "b", "b_occ")}
    meta = {"N": f.N, "cnt": [int(c) for c in f.cnt], "pri": f.pri}
    f.close()
    return {"text": text, "pats": pats, "first": first, "second": second, "regrown": regrown, "index": host_index, "meta": meta}


def test_the_inputs_reach_every_stage(passes):
    r = passes["first"]
    assert r["query_batch"]["total_hits"] > Q // 2 and (np.diff(r["query_batch"]["offsets_index"].astype(np.int64)) == 2).sum() >= 4
    assert r["query_mismatch"]["hits_by_mismatch"][1] >= Q // 2
    assert r["seeds"]["positions"].size > Q and r["chains"]["anchors"].size >= r["chains"]["chains"].size > Q // 2
    assert r["align"]["alignments"].size == r["align"]["chains"].size and r["align"]["cigar"].size >= r["align"]["chains"].size
    assert r["map"]["select_report"]["mapped"] > Q // 2 and r["map"]["hits"].size > r["map"]["select_report"]["mapped"]


def test_second_pass_in_reverse_order_equals_the_first(passes):
    for name in CALLS:
        _same(passes["first"][name], passes["second"][name], name)


def test_query_after_the_pool_was_regrown_equals_the_first(passes):
    a, b = passes["first"]["query_batch"], passes["regrown"]
    assert b["beg"].size == 4 * Q
    cut = int(a["offsets_index"][Q])
    assert cut == a["offsets"].size
    for k, n in (("beg", Q), ("end", Q), ("offsets_index", Q + 1), ("offsets", cut)):
        assert np.array_equal(a[k], b[k][:n]), k


def _view(passes):
    from kiss_amd import _lib
    v = _lib.FmiView()
    v.n_sa, v.pri, v.sa_intv = passes["meta"]["N"], passes["meta"]["pri"], 4
    for c in range(4):
        v.cnt[c] = passes["meta"]["cnt"][c]
    for k, a in passes["index"].items():
        setattr(v, k, a.ctypes.data)
    return v


def test_every_result_equals_the_host_entry_on_a_context_of_its_own(passes):
    import kiss_amd
    from kiss_amd import _lib
    from kiss_amd.sorter import _check
    lib = kiss_amd.load()
    text, pats, first = passes["text"], np.ascontiguousarray(passes["pats"]), passes["first"]
    vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    ptr = lambda a: vp(a.ctypes.data)  # noqa: E731
    v = _view(passes)

    want = first["query_batch"]
    cap = want["offsets"].size
    beg, end, offsets, oidx = np.zeros(Q, np.uint32), np.zeros(Q, np.uint32), np.zeros(cap, np.uint32), np.zeros(Q + 1, np.uint64)
    tot, chk = u64(), u64()
    lib.kiss_hip_fmi_query_batch_host.restype = ctypes.c_int
    _check(lib.kiss_hip_fmi_query_batch_host(ctypes.byref(v), ptr(pats), u32(L), u64(Q), ptr(beg), ptr(end), ctypes.byref(tot),
                                             ctypes.byref(chk), ptr(offsets), ptr(oidx), u64(cap), ctypes.c_int(0)),
           "kiss_hip_fmi_query_batch_host")
    got = {"beg": beg, "end": end, "offsets": offsets, "offsets_index": oidx, "total_hits": int(tot.value), "checksum": int(chk.value)}
    _same(want, got, "query_batch_host")

    want = first["query_mismatch"]
    cap = want["positions"].size
    counts, pos, mism, idx = np.zeros((Q, 3), np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(Q + 1, np.uint64)
    rep = _lib.FmiMmReport()
    _check(lib.kiss_hip_fmi_query_mm_host(ctypes.byref(v), ptr(pats), L, Q, 2, ptr(counts), ptr(pos), ptr(mism), ptr(idx), cap,
                                          ctypes.byref(rep), 0), "kiss_hip_fmi_query_mm_host")
    for k, a in (("counts", counts), ("positions", pos), ("mismatches", mism), ("index", idx)):
        assert np.array_equal(want[k], a), k
    assert [int(h) for h in rep.hits] == want["report"]["hits"] and int(rep.checksum) == want["checksum"]

    want = first["seeds"]
    vex = _lib.FmiViewEx()
    vex.base, vex.lookup_len, vex.lookup = v, 0, None
    reads, ridx = pats.reshape(-1), np.arange(0, (Q + 1) * L, L, dtype=np.uint64)
    nseeds, npos = want["seeds"].size, want["positions"].size
    seeds, sidx = np.zeros((nseeds, 4), np.uint32), np.zeros(2 * Q + 1, np.uint64)
    pos, pidx = np.zeros(npos, np.uint32), np.zeros(nseeds + 1, np.uint64)
    srep = _lib.FmiSeedReport()
    _check(lib.kiss_hip_fmi_seeds_host(ctypes.byref(vex), ptr(reads), ptr(ridx), Q, 19, 0, 500, 1, None, ptr(seeds), ptr(sidx), nseeds,
                                       ptr(pos), ptr(pidx), npos, ctypes.byref(srep), 0), "kiss_hip_fmi_seeds_host")
    for j, name in enumerate(("start", "len", "sa_beg", "sa_end")):
        assert np.array_equal(want["seeds"][name], seeds[:, j]), name
    for k, a in (("seed_index", sidx), ("positions", pos), ("pos_index", pidx)):
        assert np.array_equal(want[k], a), k
    assert {k: x for k, x in srep.as_dict().items() if not k.startswith("ms_")} == \
        {k: x for k, x in want["report"].items() if not k.startswith("ms_")}

    want = first["chains"]
    got = kiss_amd.chain_seeds(first["seeds"]["seeds"], first["seeds"]["seed_index"], first["seeds"]["positions"],
                               first["seeds"]["pos_index"], want_anchors=True)
    _same({k: x for k, x in want.items() if k != "seed_report"}, got, "chain_host")

    want = first["align"]
    got = kiss_amd.align_chains(text, list(pats), want["chains"], want["chain_index"], both_strands=True)
    _same({"alignments": want["alignments"], "cigar": want["cigar"], "cigar_index": want["cigar_index"], "report": want["align_report"]},
          got, "align_host")

    want = first["map"]
    got = kiss_amd.select_alignments(want["alignments"], want["chain_index"], np.full(Q, L), both_strands=True)
    _same({"hits": want["hits"], "hit_index": want["hit_index"], "report": want["select_report"]}, got, "select_host")
