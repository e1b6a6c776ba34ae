"""GPU tests of the FM-index over byte texts (FMIndexBytes / kiss_hip_fmi8_*) against the text itself
(tests/fm8_model.py: bytes.find).  No tolerances: counts, index, positions, totals and checksum are compared element by
element, for every text family x length x sa_intv, with both lane layouts of the search.

Patterns per text: on the small texts a few dozen, on the 3 * 2^20 + 5 text 2000.  The texts of one or two byte values and
the periodic ones answer a short pattern with up to n hits, and the yardstick walks every hit in Python.  So the special
patterns (absent byte, last L bytes, whole text, longer than the text) come first, the cheapest first, and are kept while
the hits of the list stay within HIT_BUDGET (one of them has some 3 * 2^20 hits on those texts); a pattern cut from the
text at random is kept if it has at most GENERIC_HIT_CAP hits and fits what is left of the budget."""
import ctypes
import functools

import numpy as np
import pytest

from tests import fm8_model as m

pytestmark = pytest.mark.gpu

SA_INTVS = (1, 2, 4, 7, 32)
SIZES = (0, 1, 2, 255, 256, 257, 65535, 65537, 3 * 2 ** 20 + 5)
FAMILIES = ("one_byte", "00_ff", "uniform256", "zipf64", "english", "period3", "period400")
HIT_BUDGET = 4_000_000
GENERIC_HIT_CAP = 20_000


@functools.lru_cache(maxsize=None)
def texts(n):
    return m.families(n, 100 + n % 1000)


def hits_up_to(S, P, limit):
    """the number of hits of P, counted no further than limit + 1"""
    count, at = 0, S.find(P)
    while at >= 0 and count <= limit:
        count += 1
        at = S.find(P, at + 1)
    return count


@functools.lru_cache(maxsize=None)
def case(family, n):
    """(text, patterns, what brute force says about them)"""
    S = texts(n)[family]
    count = 2000 if n > 1_000_000 else 40
    pats = m.patterns_for(S, count, n % 977 + len(family))
    generic = pats[:count] if n else []
    special = sorted(pats[len(generic):], key=lambda P: hits_up_to(S, P, HIT_BUDGET))  # the cheapest first
    kept, hits = [], 0
    for i, P in enumerate(special + generic):
        room = HIT_BUDGET - hits if i < len(special) else min(HIT_BUDGET - hits, GENERIC_HIT_CAP)
        h = hits_up_to(S, P, room)
        if kept and h > room:
            continue
        kept.append(P)
        hits += h
    return S, kept, m.brute_batch(S, kept)


@functools.lru_cache(maxsize=None)
def model_sa(family, n):
    return m.exact_sa_doubling(texts(n)[family])


@functools.lru_cache(maxsize=2)
def lib_sa(family, n):
    import kiss_amd
    return kiss_amd.suffix_array_bytes(texts(n)[family])


def check_answers(res, want, where):
    counts, index, positions, checksum = want
    assert np.array_equal(res["counts"], counts), where
    assert np.array_equal(res["end"].astype(np.int64) - res["beg"].astype(np.int64), counts.astype(np.int64)), where
    assert res["total_hits"] == int(counts.sum()), where
    if "positions" in res:
        assert np.array_equal(res["index"], index), where
        assert np.array_equal(res["positions"], positions), where
        assert res["checksum"] == checksum, where
        assert res["report"]["walk_failures"] == 0


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("family", FAMILIES)
def test_answers_equal_brute_force(family, n):
    from kiss_amd import FMIndexBytes
    S, pats, want = case(family, n)
    sa = lib_sa(family, n)
    first = None
    for sa_intv in SA_INTVS:
        fm = FMIndexBytes(sa_intv=sa_intv).build(S, sa=sa)
        res = fm.query_batch(pats)
        check_answers(res, want, (family, n, sa_intv))
        check_answers(fm.query_batch(pats, want_positions=False), want, (family, n, sa_intv, "counts only"))
        if first is None:
            first = res
        else:  # no result depends on sa_intv
            assert np.array_equal(res["beg"], first["beg"]) and np.array_equal(res["end"], first["end"])
        fm.close()


@pytest.mark.parametrize("n", (0, 1, 257, 65537, 3 * 2 ** 20 + 5))
@pytest.mark.parametrize("family", FAMILIES)
def test_group_layout_equals_lane_layout(family, n, monkeypatch):
    # the 16-lanes-per-pattern search of the hooks build (KISS_HIP_FM8_GROUP) against the same brute force
    from kiss_amd import FMIndexBytes
    S, pats, want = case(family, n)
    fm = FMIndexBytes(sa_intv=4, hooks=True).build(S, sa=lib_sa(family, n))
    lane = fm.query_batch(pats)
    monkeypatch.setenv("KISS_HIP_FM8_GROUP", "1")
    group = fm.query_batch(pats)
    monkeypatch.delenv("KISS_HIP_FM8_GROUP")
    check_answers(lane, want, (family, n, "lane"))
    check_answers(group, want, (family, n, "group"))
    assert np.array_equal(lane["beg"], group["beg"]) and np.array_equal(lane["end"], group["end"])
    assert lane["report"]["lf_pairs"] == group["report"]["lf_pairs"] > 0 or n == 0
    fm.close()


def arrays_of(fm):
    z = fm._sizes()
    get = lambda t, k, dt: t[:z[k]].cpu().numpy().view(dt)  # noqa: E731
    out = {"C": get(fm.C, "C", np.uint32), "map": get(fm.map, "map", np.uint8), "bwt": get(fm.bwt, "bwt_bytes", np.uint8),
           "occ1": get(fm.occ1, "occ1_entries", np.uint32), "occ2": get(fm.occ2, "occ2_entries", np.uint16),
           "sa": get(fm.sa, "sa_entries", np.uint32)}
    if fm.sa_intv != 1:
        out["b"] = get(fm.b, "b_words", np.uint64)
        out["b_occ"] = get(fm.b_occ, "b_occ_entries", np.uint32)
    return out


@pytest.mark.parametrize("sa_intv", SA_INTVS)
@pytest.mark.parametrize("n", (0, 1, 2, 255, 256, 257, 65535, 65537))
def test_arrays_equal_the_model(n, sa_intv):
    from kiss_amd import FMIndexBytes
    for family, S in texts(n).items():
        model = m.Model(S, sa_intv, SA=model_sa(family, n))
        fm = FMIndexBytes(sa_intv=sa_intv).build(S)  # (the library's own sort)
        a = arrays_of(fm)
        N = n + 1
        assert (fm.N, fm.pri, fm.sigma) == (N, model.pri, model.sigma), family
        assert np.array_equal(a["C"], model.C) and np.array_equal(a["map"], model.map), family
        assert np.array_equal(a["bwt"][:N], model.bwt) and not a["bwt"][N:].any(), family
        assert np.array_equal(a["sa"], model.sa), family
        # the rank directory against plain counting: occ1 + occ2 = occurrences of every code in front of each block
        nblk, nsb = N // 256 + 1, N // 65536 + 1
        codes = model.map[model.bwt].astype(np.int64)
        codes[model.pri] = -1
        for c in range(model.sigma):
            before = np.concatenate(([0], np.cumsum(codes == c)))[np.minimum(np.arange(nblk) * 256, N)]
            occ1 = a["occ1"][c * nsb:(c + 1) * nsb].astype(np.int64)
            occ2 = a["occ2"][c * nblk:(c + 1) * nblk].astype(np.int64)
            assert np.array_equal(occ1[np.arange(nblk) // 256] + occ2, before), (family, c)
            assert np.array_equal(occ1, before[::256]), (family, c)
        if sa_intv != 1:
            bits = np.unpackbits(a["b"].view(np.uint8), bitorder="little")[:N].astype(bool)
            assert np.array_equal(bits, model.sampled), family
            assert np.array_equal(a["b_occ"], np.concatenate(([0], np.cumsum(model.sampled)))[np.arange(N // 64 + 1) * 64]), family
        # build from a given SA = build from the library's own sort
        given = arrays_of(FMIndexBytes(sa_intv=sa_intv).build(np.frombuffer(S, np.uint8), sa=model.SA))
        assert all(np.array_equal(a[k], given[k]) for k in a), family
        fm.close()


def test_device_tensor_input_and_single_pattern_calls():
    import torch
    from kiss_amd import FMIndexBytes
    S = m.english_like(5000, 3)
    d_S = torch.from_numpy(np.frombuffer(S, np.uint8).copy()).cuda()
    fm = FMIndexBytes().build(d_S)
    assert fm.count(b"the ") == len(m.brute(S, b"the ")) > 0
    assert fm.locate(b"suffix").tolist() == m.brute(S, b"suffix")
    assert fm.count(b"\x00") == 0 and fm.locate(S + b"!").size == 0
    pats = [b"index", b"a", b"zzz"]
    concat = np.frombuffer(b"".join(pats), np.uint8)
    res = fm.query_batch((concat, np.array([0, 5, 6, 9], np.uint64)))
    check_answers(res, m.brute_batch(S, pats), "pair input")
    assert fm.query_batch([])["total_hits"] == 0 and fm.query_batch([])["index"].tolist() == [0]
    with pytest.raises(ValueError):
        fm.query_batch([b"a", b""])
    with pytest.raises(ValueError):
        fm.query_batch((concat, np.array([0, 6, 5, 9], np.uint64)))
    with pytest.raises(ValueError):
        FMIndexBytes(sa_intv=33)


@pytest.mark.parametrize("sa_intv", (1, 4, 32))
def test_serialisation_round_trip_and_rejections(tmp_path, sa_intv):
    from kiss_amd import FMIndexBytes
    S, pats, want = case("zipf64", 65537)
    fm = FMIndexBytes(sa_intv=sa_intv).build(S)
    blob = fm.to_bytes()
    back = FMIndexBytes.from_bytes(blob)
    assert (back.N, back.pri, back.sigma, back.sa_intv) == (fm.N, fm.pri, fm.sigma, sa_intv)
    check_answers(back.query_batch(pats), want, "from_bytes")
    assert back.to_bytes() == blob
    path = str(tmp_path / "t.fmi8")
    fm.save(path)
    check_answers(FMIndexBytes.load(path).query_batch(pats), want, "load")
    for bad, what in ((b"XISSFMI8" + blob[8:], "magic"), (blob[:8] + b"\x02" + blob[9:], "version"), (blob[:-1], "truncated"),
                      (blob[:40], "truncated"), (blob[:10], "truncated"), (blob + b"\x00", "trailing")):
        with pytest.raises(ValueError, match=what):
            FMIndexBytes.from_bytes(bad)


def _np_ptr(a):
    return ctypes.c_void_p(a.ctypes.data if a is not None and a.size else None)


def host_build(S, sa_intv, SA=None):
    """kiss_hip_fmi8_build_host through ctypes -> (arrays, sigma, pri)"""
    import kiss_amd
    from kiss_amd import _lib
    lib = kiss_amd.load()
    a = np.frombuffer(S, np.uint8)
    sigma, pri = ctypes.c_uint32(), ctypes.c_uint32()
    none = ctypes.c_void_p()
    assert lib.kiss_hip_fmi8_build_host(_np_ptr(a), a.size, none, sa_intv, 0, none, none, none, none, none, none, none, none,
                                        ctypes.byref(sigma), ctypes.byref(pri), 0) == 0
    z = m.sizes(a.size, sa_intv, sigma.value)
    arr = {"C": np.zeros(257, np.uint32), "map": np.zeros(256, np.uint8), "bwt": np.zeros(z["bwt_bytes"] + 16, np.uint8),
           "occ1": np.zeros(z["occ1_entries"] + 1, np.uint32), "occ2": np.zeros(z["occ2_entries"] + 1, np.uint16),
           "sa": np.zeros(z["sa_entries"], np.uint32), "b": np.zeros(z["b_words"] + 1, np.uint64),
           "b_occ": np.zeros(z["b_occ_entries"] + 1, np.uint32)}
    rc = lib.kiss_hip_fmi8_build_host(_np_ptr(a), a.size, _np_ptr(SA), sa_intv, sigma.value, _np_ptr(arr["C"]), _np_ptr(arr["map"]),
                                      _np_ptr(arr["bwt"]), _np_ptr(arr["occ1"]), _np_ptr(arr["occ2"]), _np_ptr(arr["sa"]),
                                      _np_ptr(arr["b"]), _np_ptr(arr["b_occ"]), ctypes.byref(sigma), ctypes.byref(pri), 0)
    assert rc == 0, rc
    for k, key in (("bwt", "bwt_bytes"), ("occ1", "occ1_entries"), ("occ2", "occ2_entries"), ("b", "b_words"), ("b_occ", "b_occ_entries")):
        arr[k] = arr[k][:z[key]]
    return arr, sigma.value, pri.value, _lib


def host_view(arr, N, sigma, pri, sa_intv, _lib):
    v = _lib.Fmi8View()
    v.n_sa, v.pri, v.sa_intv, v.sigma = N, pri, sa_intv, sigma
    for k in ("C", "map", "bwt", "occ1", "occ2", "sa"):
        setattr(v, k, arr[k].ctypes.data)
    if sa_intv != 1:
        v.b, v.b_occ = arr["b"].ctypes.data, arr["b_occ"].ctypes.data
    return v


def host_query(v, pats, want_positions, capacity=None):
    import kiss_amd
    from kiss_amd import _lib
    lib = kiss_amd.load()
    concat = np.frombuffer(b"".join(pats), np.uint8)
    pidx = np.zeros(len(pats) + 1, np.uint64)
    np.cumsum([len(p) for p in pats], out=pidx[1:])
    Q = len(pats)
    beg, end = np.zeros(Q + 1, np.uint32), np.zeros(Q + 1, np.uint32)
    tot, chk, rep = ctypes.c_uint64(), ctypes.c_uint64(), _lib.Fmi8Report()
    rc = lib.kiss_hip_fmi8_query_host(ctypes.byref(v), _np_ptr(concat), _np_ptr(pidx), Q, _np_ptr(beg), _np_ptr(end), ctypes.byref(tot),
                                      ctypes.byref(chk), None, None, 0, ctypes.byref(rep), 0)
    res = {"rc": rc, "beg": beg[:Q], "end": end[:Q], "counts": (end[:Q] - beg[:Q]).astype(np.uint64), "total_hits": tot.value}
    if rc == 0 and want_positions:
        cap = tot.value if capacity is None else capacity
        positions, index = np.zeros(cap + 1, np.uint32), np.zeros(Q + 1, np.uint64)
        rc = lib.kiss_hip_fmi8_query_host(ctypes.byref(v), _np_ptr(concat), _np_ptr(pidx), Q, _np_ptr(beg), _np_ptr(end),
                                          ctypes.byref(tot), ctypes.byref(chk), _np_ptr(positions), _np_ptr(index), cap, ctypes.byref(rep), 0)
        res.update(rc=rc, positions=positions[:tot.value], index=index, checksum=chk.value, total_hits=tot.value,
                   report=rep.as_dict())
    return res


@pytest.mark.parametrize("sa_intv", (1, 4, 7))
def test_host_entry_points_equal_the_device_ones(sa_intv):
    from kiss_amd import FMIndexBytes
    for family, n in (("english", 65537), ("00_ff", 257), ("uniform256", 0), ("one_byte", 1)):
        S, pats, want = case(family, n)
        arr, sigma, pri, _lib = host_build(S, sa_intv)  # (SA_or_null == NULL: sorts first)
        fm = FMIndexBytes(sa_intv=sa_intv).build(S)
        dev = arrays_of(fm)
        assert (sigma, pri) == (fm.sigma, fm.pri)
        assert all(np.array_equal(arr[k], dev[k]) for k in dev), family
        arr2 = host_build(S, sa_intv, SA=lib_sa(family, n))[0]
        assert all(np.array_equal(arr[k], arr2[k]) for k in dev), family
        res = host_query(host_view(arr, n + 1, sigma, pri, sa_intv, _lib), pats, True)
        assert res["rc"] == 0
        check_answers(res, want, (family, "host"))
        fm.close()


def test_host_query_empty_batch_and_size_then_fill():
    import kiss_amd
    S = b"abracadabra" * 50
    arr, sigma, pri, _lib = host_build(S, 4)
    v = host_view(arr, len(S) + 1, sigma, pri, 4, _lib)
    index, tot, chk = np.full(1, 7, np.uint64), ctypes.c_uint64(9), ctypes.c_uint64(9)
    pos = np.zeros(1, np.uint32)
    rc = kiss_amd.load().kiss_hip_fmi8_query_host(ctypes.byref(v), None, None, 0, None, None, ctypes.byref(tot), ctypes.byref(chk),
                                                  _np_ptr(pos), _np_ptr(index), 0, None, 0)  # Q = 0: index[0] = 0
    assert rc == 0 and index.tolist() == [0] and (tot.value, chk.value) == (0, 0)
    pats = [b"a", b"zz", b"abra"]  # many hits, none, some
    want = [m.brute(S, p) for p in pats]
    total = sum(len(w) for w in want)
    res = host_query(v, pats, True, capacity=0)  # the sizing call: the total comes back
    assert res["rc"] == _lib.KISS_HIP_E_INVALID and res["total_hits"] == total and res["report"]["hits"] == total
    res = host_query(v, pats, True, capacity=total)
    assert res["rc"] == 0 and res["index"].tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert res["positions"].tolist() == [p for w in want for p in w]


def test_error_codes():
    import torch
    import kiss_amd
    from kiss_amd import FMIndexBytes, _lib
    lib = kiss_amd.load()
    S = b"abracadabra" * 50
    fm = FMIndexBytes(sa_intv=4).build(S)
    ctx = fm._context(1 << 20)
    vp = ctypes.c_void_p

    def dev(a):
        return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else a.dtype).copy()).cuda()

    def query(view, pats_concat, pidx, Q, positions=None, index=None, cap=0, beg_null=False):
        d_pat, d_pidx = dev(np.frombuffer(pats_concat, np.uint8)), dev(np.array(pidx, np.uint64))
        beg, end = torch.zeros(Q + 1, dtype=torch.int32).cuda(), torch.zeros(Q + 1, dtype=torch.int32).cuda()
        tot, chk, rep = ctypes.c_uint64(), ctypes.c_uint64(), _lib.Fmi8Report()
        rc = lib.kiss_hip_fmi8_query_dev(ctx._ctx, ctypes.byref(view), vp(d_pat.data_ptr()), vp(d_pidx.data_ptr()), Q,
                                         None if beg_null else vp(beg.data_ptr()), vp(end.data_ptr()), ctypes.byref(tot),
                                         ctypes.byref(chk), positions, index, cap, ctypes.byref(rep), None)
        return rc, tot.value, rep

    v = fm._view()
    assert query(v, b"abra", [0, 4], 1)[:2] == (0, len(m.brute(S, b"abra")))
    assert query(v, b"abra", [0, 0, 4], 2)[0] == _lib.KISS_HIP_E_INVALID          # a zero-length pattern
    assert query(v, b"abra", [0, 3, 2, 4], 3)[0] == _lib.KISS_HIP_E_INVALID       # pat_index decreases
    assert query(v, b"abra", [0, 4], 1, beg_null=True)[0] == _lib.KISS_HIP_E_INVALID  # a required pointer NULL
    assert query(v, b"abra", [0, 4], 0)[:2] == (0, 0)                             # Q == 0
    assert query(v, S + b"a", [0, len(S) + 1], 1)[:2] == (0, 0)                   # L > n
    pos, idx = torch.zeros(4096, dtype=torch.int32).cuda(), torch.zeros(8, dtype=torch.int64).cuda()
    assert query(v, b"abra", [0, 4], 1, vp(pos.data_ptr()), None, 100)[0] == _lib.KISS_HIP_E_INVALID  # positions without index
    total = len(m.brute(S, b"a"))
    rc, tot, rep = query(v, b"a", [0, 1], 1, vp(pos.data_ptr()), vp(idx.data_ptr()), total - 1)  # capacity too small
    assert (rc, tot, rep.hits) == (_lib.KISS_HIP_E_INVALID, total, total)
    rc, tot, rep = query(v, b"a", [0, 1], 1, vp(pos.data_ptr()), vp(idx.data_ptr()), total)
    assert (rc, tot) == (0, total) and pos[:total].cpu().numpy().tolist() == m.brute(S, b"a")
    for bad in (0, 33):  # sa_intv outside 1..32
        w = fm._view()
        w.sa_intv = bad
        assert query(w, b"abra", [0, 4], 1)[0] == _lib.KISS_HIP_E_UNSUPPORTED
    sigma, pri = ctypes.c_uint32(), ctypes.c_uint32()
    d_S = dev(np.frombuffer(S, np.uint8))
    assert lib.kiss_hip_fmi8_build_dev(ctx._ctx, vp(d_S.data_ptr()), len(S), None, 33, 0, None, None, None, None, None, None, None,
                                       None, ctypes.byref(sigma), ctypes.byref(pri), None) == _lib.KISS_HIP_E_UNSUPPORTED
    assert lib.kiss_hip_fmi8_build_dev(ctx._ctx, vp(d_S.data_ptr()), len(S), None, 4, 0, None, None, None, None, None, None, None,
                                       None, None, ctypes.byref(pri), None) == _lib.KISS_HIP_E_INVALID
    # arrays sized for fewer symbols than the text holds: refused, with the number needed
    d_SA = dev(kiss_amd.suffix_array_bytes(S).view(np.int32))
    rc = lib.kiss_hip_fmi8_build_dev(ctx._ctx, vp(d_S.data_ptr()), len(S), vp(d_SA.data_ptr()), 4, 2, vp(fm.C.data_ptr()),
                                     vp(fm.map.data_ptr()), vp(fm.bwt.data_ptr()), vp(fm.occ1.data_ptr()), vp(fm.occ2.data_ptr()),
                                     vp(fm.sa.data_ptr()), vp(fm.b.data_ptr()), vp(fm.b_occ.data_ptr()), ctypes.byref(sigma),
                                     ctypes.byref(pri), None)
    assert (rc, sigma.value) == (_lib.KISS_HIP_E_INVALID, 5)
    fm.close()


def test_more_hits_than_the_sort_arrays_hold():
    import torch
    import kiss_amd
    from kiss_amd import FMIndexBytes, _lib
    n = 1_500_000
    S = b"a" * n
    fm = FMIndexBytes(sa_intv=4).build(S)
    # the C call says so, with the totals
    lib = kiss_amd.load()
    with kiss_amd.Context(max_n=1 << 20) as small:
        v = fm._view()
        d_pat = torch.from_numpy(np.frombuffer(b"a", np.uint8).copy()).cuda()
        d_pidx = torch.tensor([0, 1], dtype=torch.int64).cuda()
        beg, end = torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
        pos, idx = torch.zeros(n, dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
        tot, chk, rep = ctypes.c_uint64(), ctypes.c_uint64(), _lib.Fmi8Report()
        vp = ctypes.c_void_p
        rc = lib.kiss_hip_fmi8_query_dev(small._ctx, ctypes.byref(v), vp(d_pat.data_ptr()), vp(d_pidx.data_ptr()), 1, vp(beg.data_ptr()),
                                         vp(end.data_ptr()), ctypes.byref(tot), ctypes.byref(chk), vp(pos.data_ptr()), vp(idx.data_ptr()),
                                         n, ctypes.byref(rep), None)
        assert (rc, tot.value, rep.hits) == (_lib.KISS_HIP_E_UNSUPPORTED, n, n)
    # the class splits the batch and comes back complete
    pats = [b"a", b"aa", b"a" * 300, b"b", b"aaa"]
    res = fm.query_batch(pats)
    assert res["counts"].tolist() == [n, n - 1, n - 299, 0, n - 2]
    assert res["report"]["calls"] > 1
    at = 0
    for c in res["counts"].tolist():
        assert np.array_equal(res["positions"][at:at + c], np.arange(c, dtype=np.uint32))
        at += c
    assert res["index"].tolist() == [0] + np.cumsum(res["counts"]).tolist()
    assert res["checksum"] == int(res["positions"].astype(np.uint64).sum())
    fm.close()


def test_the_whole_text_as_a_pattern_at_3m():
    from kiss_amd import FMIndexBytes
    n = 3 * 2 ** 20 + 5
    S = texts(n)["english"]
    fm = FMIndexBytes(sa_intv=7).build(S, sa=lib_sa("english", n))
    pats = [S, S[1:], S[:-1], S[5:5 + 2 ** 20], S + b"a"]
    check_answers(fm.query_batch(pats), m.brute_batch(S, pats), "whole text")
    fm.close()


def test_cross_check_against_the_dna_index():
    # a DNA text written as the bytes A C G T: the same counts and position sets as the shipped DNA index gives
    from kiss_amd import FMIndexBytes
    from kiss_amd.fm_index import FMIndex
    from tests import gen
    codes = gen.genome_like(300_000, 8)
    S = np.frombuffer(b"ACGT", np.uint8)[codes].tobytes()
    rng = np.random.default_rng(4)
    dna = FMIndex().build(codes, exact=True)
    fm8 = FMIndexBytes().build(S)
    for L in (1, 5, 12, 32, 100):
        starts = rng.integers(0, codes.size - L, 400)
        pats = np.stack([codes[p:p + L] for p in starts]).astype(np.uint8)
        pats[::5, L // 2] = (pats[::5, L // 2] + 1) % 4  # some with one base changed
        a = dna.query_mismatch(pats, 0)
        b = fm8.query_batch([np.frombuffer(b"ACGT", np.uint8)[p].tobytes() for p in pats])
        assert np.array_equal(a["counts"][:, 0].astype(np.uint64), b["counts"])
        assert np.array_equal(a["index"], b["index"])
        assert np.array_equal(a["positions"], b["positions"])
    dna.close()
    fm8.close()
