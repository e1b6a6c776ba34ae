"""LCP arrays on the device (kiss_hip_ctx_lcp_dna_u32_dev / _u8_dev and the one-shots): Kasai on small and medium
texts, the hash check on large ones, the byte path's no-over-read rule, input checks, workspace, both libraries."""
import numpy as np
import pytest

from tests import gen, lcp_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


def to_dev(torch_dev, a):
    torch, dev = torch_dev
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(dev)


def from_dev(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 else a


def planted(n, seed, copy_len=100_000, copies=3):
    S = gen.iid(n, seed)
    rng = np.random.default_rng(seed)
    src = int(rng.integers(0, n - copy_len))
    for _ in range(copies):
        dst = int(rng.integers(0, n - copy_len))
        S[dst:dst + copy_len] = S[src:src + copy_len].copy()
    return S


def dna_texts():
    out = {"n0": np.zeros(0, np.uint8), "n1": gen.iid(1, 1), "n2": gen.iid(2, 2), "n2AA": np.zeros(2, np.uint8),
           "allA5000": np.zeros(5000, np.uint8), "AC3001": np.tile(np.array([0, 1], np.uint8), 3001)[:6001],
           "period7": gen.periodic(7007, 7, 3), "periodic_mut": gen.periodic(300_000, 171, 4, 40),
           "periodic3_mut": gen.periodic(100_000, 3, 5, 7), "genome200k": gen.genome_like(200_000, 6),
           "genome2M": gen.genome_like(2_000_000, 7), "planted": planted(600_000, 8)}
    for n in (31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 4095, 4096, 4097, 8191, 8192, 8193):
        out["iid%d" % n] = gen.iid(n, n)
        out["allA%d" % n] = np.zeros(n, np.uint8)
    return out


DNA = dna_texts()


@pytest.mark.parametrize("name", list(DNA))
def test_dna_one_shot_equals_kasai(name):
    import kiss_amd
    S = DNA[name]
    SA, LCP = kiss_amd.lcp_array(S)
    assert SA.size == S.size + 1 and LCP.size == S.size + 1
    ref_sa = kiss_amd.KISS2Sorter.get_suffix_array_dna(S, kiss_amd.K_UNBOUNDED) if S.size else np.zeros(1, np.uint32)
    assert np.array_equal(SA, ref_sa)
    assert np.array_equal(LCP, lcp_model.kasai(S, SA))
    SA2, LCP2 = kiss_amd.lcp_array(S, SA=SA)  # the same with the SA given
    assert np.array_equal(SA2, SA) and np.array_equal(LCP2, LCP)


def test_dna_device_report_and_in_place(torch_dev):
    import kiss_amd
    S = gen.genome_like(500_000, 9)
    with kiss_amd.Context(max_n=S.size) as ctx:
        d_S = to_dev(torch_dev, S)
        d_SA = to_dev(torch_dev, np.zeros(S.size + 1, np.uint32))
        ctx.suffix_sort_dev(d_S.data_ptr(), S.size, d_SA.data_ptr(), kiss_amd.K_UNBOUNDED, kiss_amd.ALGO_PREFIX_DOUBLING)
        SA = from_dev(d_SA)
        st = ctx.stats()
        d_LCP = to_dev(torch_dev, np.full(S.size + 1, 7, np.uint32))
        rep = ctx.lcp_dev(d_S.data_ptr(), S.size, d_SA.data_ptr(), d_LCP.data_ptr())
        LCP = from_dev(d_LCP)
        assert ctx.stats() == st  # the sort statistics are left alone
        ref = lcp_model.kasai(S, SA)
        assert np.array_equal(LCP, ref)
        assert rep["n"] == S.size and rep["lcp_sum"] == int(ref.astype(np.uint64).sum()) and rep["max_lcp"] == int(ref.max())
        assert 0 < rep["irreducible"] <= S.size and rep["long_pairs"] <= rep["irreducible"]
        assert rep["ms_total"] > 0 and rep["ms_total"] >= rep["ms_short"]
        rep2 = ctx.lcp_dev(d_S.data_ptr(), S.size, d_SA.data_ptr(), d_SA.data_ptr())  # in place: LCP replaces SA
        assert np.array_equal(from_dev(d_SA), ref) and rep2["lcp_sum"] == rep["lcp_sum"]


@pytest.mark.parametrize("kind", ["genome", "allA"])
def test_dna_large_hash_check(torch_dev, kind):
    import kiss_amd
    n = 130_000_000 if kind == "genome" else 100_000_000
    S = gen.genome_like(n, 11) if kind == "genome" else np.zeros(n, np.uint8)
    with kiss_amd.Context(max_n=n) as ctx:
        d_S = to_dev(torch_dev, S)
        d_SA = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        ctx.suffix_sort_dev(d_S.data_ptr(), n, d_SA.data_ptr(), kiss_amd.K_UNBOUNDED, kiss_amd.ALGO_PREFIX_DOUBLING)
        ws = ctx.workspace_bytes()
        d_LCP = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        rep = ctx.lcp_dev(d_S.data_ptr(), n, d_SA.data_ptr(), d_LCP.data_ptr())
        assert ctx.workspace_bytes() == ws
        SA, LCP = from_dev(d_SA), from_dev(d_LCP)
    del d_S, d_SA, d_LCP
    assert rep["lcp_sum"] == int(LCP.astype(np.uint64).sum()) and rep["max_lcp"] == int(LCP.max())
    if kind == "allA":
        assert np.array_equal(SA, np.arange(n, -1, -1, dtype=np.uint32))
        expect = np.arange(-1, n, dtype=np.int64)
        expect[0] = 0
        assert np.array_equal(LCP, expect.astype(np.uint32))
        assert rep["long_pairs"] >= 1 and rep["max_lcp"] == n - 1
    else:
        assert lcp_model.lcp_hash_check(S, SA, LCP)


SMALL_BYTES = [b"", b"a", b"aa", b"ab", b"ba", b"banana", b"mississippi", b"abracadabra" * 7, b"\x00\x00\x00",
               b"\x00\x01\x00\x01\x00", b"\xff" * 40, bytes(range(256)) * 3, b"aaaaaaab" * 50 + b"aaaaaaa",
               b"the quick brown fox jumps over the lazy dog " * 20]


@pytest.mark.parametrize("text", SMALL_BYTES)
def test_bytes_small_texts_equal_kasai(text):
    import kiss_amd
    SA, LCP = kiss_amd.lcp_array_bytes(text)
    S = np.frombuffer(text, np.uint8)
    assert np.array_equal(SA, lcp_model.naive_sa(S))
    assert np.array_equal(LCP, lcp_model.kasai(S, SA))


def test_bytes_random_texts_equal_kasai():
    import kiss_amd
    rng = np.random.default_rng(5)
    for case in range(60):
        n = int(rng.integers(0, 1500))
        sigma = int(rng.choice([1, 2, 3, 4, 16, 256]))
        b = rng.integers(0, sigma, n, dtype=np.uint8)
        if case % 3 == 0 and n > 50:
            a, c, ln = int(rng.integers(0, n // 2)), int(rng.integers(n // 2, n)), int(rng.integers(8, 40))
            b[c:c + ln] = b[a:a + ln][:b[c:c + ln].size]
        SA, LCP = kiss_amd.lcp_array_bytes(b.tobytes())
        assert np.array_equal(LCP, lcp_model.kasai(b, SA)), (case, n, sigma)


@pytest.mark.parametrize("n", [1, 2, 7, 9, 4099, 65_541, 1_000_003, 2_000_007])
def test_bytes_never_read_past_the_view(torch_dev, n):
    # the text is a view into a larger device buffer whose bytes behind the view repeat the text's start: reading them would
    # lengthen the lcp of every suffix that runs to the end
    import kiss_amd
    assert n % 8 != 0
    rng = np.random.default_rng(n)
    S = rng.integers(0, 3, n, dtype=np.uint8) if n > 1000 else np.zeros(n, np.uint8)
    if n > 1000:
        S[-500:] = S[:500]  # the end of the text repeats its start as well
    SA = kiss_amd.suffix_array_bytes(S)
    ref = lcp_model.kasai(S, SA)
    off = 3  # an unaligned start too
    buf = np.concatenate([np.full(off, 9, np.uint8), S, S[:64], S[:64]])
    d_buf = to_dev(torch_dev, buf)
    d_SA = to_dev(torch_dev, SA)
    d_LCP = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
    with kiss_amd.Context(max_n=n) as ctx:
        rep = ctx.lcp_dev(d_buf.data_ptr() + off, n, d_SA.data_ptr(), d_LCP.data_ptr(), alphabet="bytes")
    assert np.array_equal(from_dev(d_LCP), ref)
    assert rep["lcp_sum"] == int(ref.astype(np.uint64).sum())


def test_bytes_large_random_hash_check():
    import kiss_amd
    S = np.random.default_rng(4).integers(0, 256, 3_000_000, dtype=np.uint8)
    S[1_000_000:1_400_000] = S[2_000_000:2_400_000]
    SA, LCP = kiss_amd.lcp_array_bytes(S)
    assert lcp_model.lcp_hash_check(S, SA, LCP)
    assert int(LCP.max()) >= 400_000


def test_bad_sa_is_invalid_and_k_ordered_sa_leaves_the_device_usable(torch_dev):
    import kiss_amd
    from kiss_amd import _lib
    S = gen.genome_like(300_000, 12)
    n = S.size
    with kiss_amd.Context(max_n=n) as ctx:
        d_S = to_dev(torch_dev, S)
        d_LCP = to_dev(torch_dev, np.full(n + 1, 5, np.uint32))
        exact = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED, kiss_amd.ALGO_PREFIX_DOUBLING)
        for alphabet in ("dna", "bytes"):
            bad0 = exact.copy()
            bad0[0] = 0
            bad_range = exact.copy()
            bad_range[n // 2] = n + 1
            bad_big = exact.copy()
            bad_big[-1] = 0xFFFFFFFF
            for bad in (bad0, bad_range, bad_big):
                d_bad = to_dev(torch_dev, bad)
                with pytest.raises(_lib.KissHipError) as e:
                    ctx.lcp_dev(d_S.data_ptr(), n, d_bad.data_ptr(), d_LCP.data_ptr(), alphabet=alphabet)
                assert e.value.status == _lib.KISS_HIP_E_INVALID
            assert (from_dev(d_LCP) == 5).all()  # nothing written
        # k-ordered (not exact) and a permutation with duplicates: OK, unspecified values, in bounds
        kord = ctx.suffix_sort(S, 32, kiss_amd.ALGO_PARALLEL_SORTING)
        assert not np.array_equal(kord, exact)
        dup = exact.copy()
        dup[1:1000] = exact[1000]
        dup[5000] = n
        for sa in (kord, dup):
            ctx.lcp_dev(d_S.data_ptr(), n, to_dev(torch_dev, sa).data_ptr(), d_LCP.data_ptr())
            ctx.lcp_dev(d_S.data_ptr(), n, to_dev(torch_dev, sa).data_ptr(), d_LCP.data_ptr(), alphabet="bytes")
        # the device and the context still give right answers
        d_SA = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        ctx.suffix_sort_dev(d_S.data_ptr(), n, d_SA.data_ptr(), kiss_amd.K_UNBOUNDED, kiss_amd.ALGO_PREFIX_DOUBLING)
        assert np.array_equal(from_dev(d_SA), exact)
        ctx.lcp_dev(d_S.data_ptr(), n, d_SA.data_ptr(), d_LCP.data_ptr())
        assert np.array_equal(from_dev(d_LCP), lcp_model.kasai(S, exact))
    with pytest.raises(_lib.KissHipError):
        kiss_amd.lcp_array(S, SA=bad0)


@pytest.mark.parametrize("alphabet", ["dna", "bytes"])
def test_lcp_on_a_context_with_a_small_lms_capacity(torch_dev, alphabet):
    # kiss_hip_ctx_create_sized with a tiny LMS capacity: the scan's block maxima (n / 4096 of them) do not fit the LMS
    # arrays, and the overflow lists fill up (their pairs are then compared by the lane / wave that found them)
    import kiss_amd
    n = 30_000_000
    S = gen.periodic(n, 171, 15, 50_000)  # copies of a few hundred bases between mutations: tens of thousands of long pairs
    if alphabet == "bytes":
        S = (S * 61 + 7).astype(np.uint8)
    SA, LCP = kiss_amd.lcp_array(S) if alphabet == "dna" else kiss_amd.lcp_array_bytes(S)
    with kiss_amd.Context(max_n=n, lms_capacity=1) as ctx:
        d_S, d_SA = to_dev(torch_dev, S), to_dev(torch_dev, SA)
        d_LCP = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        rep = ctx.lcp_dev(d_S.data_ptr(), n, d_SA.data_ptr(), d_LCP.data_ptr(), alphabet=alphabet)
        assert np.array_equal(from_dev(d_LCP), LCP)
    assert rep["long_pairs"] > 4097  # more than the lists hold on this context
    assert lcp_model.lcp_hash_check(S, SA, LCP)


@pytest.mark.parametrize("alphabet", ["dna", "bytes"])
def test_lcp_after_exact_sort_allocates_nothing(torch_dev, alphabet):
    import kiss_amd
    S = gen.genome_like(1_000_000, 13) if alphabet == "dna" else np.random.default_rng(1).integers(0, 200, 1_000_000,
                                                                                                     dtype=np.uint8)
    n = S.size
    with kiss_amd.Context(max_n=n) as ctx:
        d_S = to_dev(torch_dev, S)
        d_SA = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        d_LCP = to_dev(torch_dev, np.zeros(n + 1, np.uint32))
        if alphabet == "dna":
            ctx.suffix_sort_dev(d_S.data_ptr(), n, d_SA.data_ptr(), kiss_amd.K_UNBOUNDED, kiss_amd.ALGO_PREFIX_DOUBLING)
        else:
            ctx._lib.kiss_hip_ctx_suffix_sort_u8_dev(ctx._ctx, d_S.data_ptr(), n, d_SA.data_ptr(), None)
        ws = ctx.workspace_bytes()
        ctx.lcp_dev(d_S.data_ptr(), n, d_SA.data_ptr(), d_LCP.data_ptr(), alphabet=alphabet)
        assert ctx.workspace_bytes() == ws
        assert lcp_model.lcp_hash_check(S, from_dev(d_SA), from_dev(d_LCP))


def test_both_libraries_agree():
    import kiss_amd
    S = gen.genome_like(400_000, 14)
    SA, LCP = kiss_amd.lcp_array(S)
    SA_h, LCP_h = kiss_amd.sorter.lcp_array(S, hooks=True)
    assert np.array_equal(SA, SA_h) and np.array_equal(LCP, LCP_h)
    B = np.random.default_rng(2).integers(0, 256, 200_000, dtype=np.uint8)
    a = kiss_amd.lcp_array_bytes(B)
    b = kiss_amd.sorter.lcp_array_bytes(B, hooks=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
