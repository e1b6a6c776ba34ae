"""General alphabet (bytes): the exact suffix array of kiss_hip_suffix_sort_u8 against plain Python / the DNA path."""
import numpy as np
import pytest

from tests import gen
from tests.verify_model import is_suffix_array

pytestmark = pytest.mark.gpu


def naive_sa(b):
    n = len(b)
    return np.array([n] + sorted(range(n), key=lambda i: b[i:]), dtype=np.uint32)


@pytest.mark.parametrize("text", [b"", b"a", b"aa", b"ab", b"ba", b"banana", b"mississippi", b"abracadabra" * 7,
                                  b"\x00\x00\x00", b"\x00\x01\x00\x01\x00", b"\xff" * 40, bytes(range(256)) * 3,
                                  b"aaaaaaab" * 50 + b"aaaaaaa", b"the quick brown fox jumps over the lazy dog " * 20])
def test_small_texts_against_python(text):
    import kiss_amd
    sa = kiss_amd.suffix_array_bytes(text)
    assert np.array_equal(sa, naive_sa(text))


def test_random_texts_against_python():
    import kiss_amd
    rng = np.random.default_rng(5)
    for case in range(60):
        n = int(rng.integers(0, 1500))
        sigma = int(rng.choice([1, 2, 3, 4, 16, 256]))
        b = rng.integers(0, sigma, n, dtype=np.uint8)
        if case % 3 == 0 and n > 50:  # plant repeats longer than the 7-character key
            a, c, ln = int(rng.integers(0, n // 2)), int(rng.integers(n // 2, n)), int(rng.integers(8, 40))
            b[c:c + ln] = b[a:a + ln][:b[c:c + ln].size]
        assert np.array_equal(kiss_amd.suffix_array_bytes(b.tobytes()), naive_sa(b.tobytes())), (case, n, sigma)


@pytest.mark.parametrize("kind", ["bytes", "english-like", "periodic", "dna"])
def test_large_texts_are_suffix_arrays(oracle, kind):
    import kiss_amd
    rng = np.random.default_rng(9)
    n = 2_000_000
    if kind == "bytes":
        S = rng.integers(0, 256, n, dtype=np.uint8)
    elif kind == "english-like":
        words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) + b" " for _ in range(300)]
        S = np.frombuffer(b"".join(words[int(i)] for i in rng.integers(0, 300, n // 5)), dtype=np.uint8)[:n].copy()
    elif kind == "periodic":
        S = np.tile(rng.integers(0, 256, 13, dtype=np.uint8), n // 13 + 1)[:n].copy()
    else:
        S = gen.genome_like(n, 3)
    sa = kiss_amd.suffix_array_bytes(S)
    assert is_suffix_array(S, sa)
    if kind == "dna":  # the byte path and the DNA paths agree (codes 0..3 are bytes too)
        assert np.array_equal(sa, oracle.suffix_sort(S, kiss_amd.K_UNBOUNDED))


@pytest.mark.parametrize("values", [b"ABCD", b"ACT", b"\x00\xff", b"z", b"\x05\x06\x07\x08"])
def test_texts_over_at_most_four_values_take_the_dna_path(oracle, monkeypatch, values):
    # general.hip maps such a text to codes 0..3 in value order and sorts it as DNA (exact order); the answer is the
    # one the 7-character path gives (KISS_HIP_NO_SMALL_ALPHABET=1) and the oracle's exact suffix array of the codes
    import kiss_amd
    codes = gen.genome_like(300_000, 3) % len(values) if len(values) > 1 else np.zeros(20_000, np.uint8)
    if codes.size > 60_000:
        codes[1000:1600] = codes[50_000:50_600]  # a copy longer than any key
    text = np.frombuffer(values, np.uint8)[codes]
    sa = kiss_amd.suffix_array_bytes(text.tobytes())
    assert is_suffix_array(text, sa)
    assert np.array_equal(sa, oracle.suffix_sort(codes.astype(np.uint8), 0xFFFFFFFF))
    monkeypatch.setenv("KISS_HIP_NO_SMALL_ALPHABET", "1")  # (a switch of the hooks build)
    assert np.array_equal(kiss_amd.suffix_array_bytes(text.tobytes(), hooks=True), sa)


# ---- sizes and dispatch edges between 1500 and 2 M -----------------------------------------------------------------
K_UNBOUNDED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.fixture(scope="module")
def gctx():
    import kiss_amd
    c = kiss_amd.Context(max_n=1_000_003, device=0)
    yield c
    c.close()


def sort_u8_on(c, torch_dev, S):
    """kiss_hip_ctx_suffix_sort_u8_dev on the context c; the result has to pass the device's exactness proof
    (tests/test_verify_mutations_gpu.py tests that proof) -> the suffix array in host memory"""
    import ctypes
    torch, dev = torch_dev
    n = S.size
    d_S = torch.from_numpy(np.ascontiguousarray(S, dtype=np.uint8)).to(dev)
    d_SA = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rc = c._lib.kiss_hip_ctx_suffix_sort_u8_dev(c._ctx, ctypes.c_void_p(d_S.data_ptr() if n else 0), n,
                                                ctypes.c_void_p(d_SA.data_ptr()), None)
    assert rc == 0
    rep = c.verify_sa_dev(d_S.data_ptr() if n else 0, n, d_SA.data_ptr(), K_UNBOUNDED)
    assert rep["ok"] == 1 and rep["exact"] == 1, rep
    return d_SA.cpu().numpy().view(np.uint32)


def check_bytes_sa(S, sa, oracle=None):
    """naive_sa where n <= 20 000, the linear-time proof above that, the oracle on texts of DNA codes; and the LCP array
    of the byte path against Kasai's where n <= 300 000"""
    import kiss_amd
    from tests import lcp_model
    n = S.size
    if n <= 20_000:
        assert np.array_equal(sa, naive_sa(S.tobytes()))
    else:
        assert is_suffix_array(S, sa)
    if oracle is not None and n and int(S.max()) <= 3:
        assert np.array_equal(sa, oracle.suffix_sort(S, K_UNBOUNDED))
    if n <= 300_000:
        sa2, lcp = kiss_amd.lcp_array_bytes(S)
        assert np.array_equal(sa2, sa)
        assert np.array_equal(lcp, lcp_model.kasai(S, sa))


@pytest.mark.parametrize("sigma", [1, 2, 4, 5, 16, 256])
@pytest.mark.parametrize("n", [6, 7, 8, 4095, 4096, 4097, 65_535, 65_536, 65_537, 262_145, 700_001])
def test_sizes_and_alphabets_at_the_dispatch_edges(gctx, torch_dev, oracle, n, sigma):
    # n = 7: the 7-character key (rank doubling only for n >= 7); n = 4096: the presence scan and, for at most four
    # values, the DNA path; sigma 4 | 5: that switch; 65 536 +- 1, 262 145, 700 001: tile sizes of the radix sort
    S = np.random.default_rng(1000 * sigma + n % 997).integers(0, sigma, n, dtype=np.uint8)
    if n > 100:
        assert np.unique(S).size == sigma
    check_bytes_sa(S, sort_u8_on(gctx, torch_dev, S), oracle)


# k_ga_presence: blocks = min(4096, ceil(n / (64 * 4 * 64))) workgroups of 4 waves; wave w reads the 64-byte chunks
# c = w, w + W, w + 2 W, ... with W = 4 * blocks.  n = 1 000 000: blocks = ceil(1 000 000 / 16 384) = 62, W = 248.
PRESENCE_WAVES_1M = 4 * (-(-1_000_000 // 16_384))


@pytest.mark.parametrize("waves", [PRESENCE_WAVES_1M - 1, PRESENCE_WAVES_1M, PRESENCE_WAVES_1M + 1])
def test_more_than_four_values_that_no_single_wave_sees_together(gctx, torch_dev, monkeypatch, waves):
    # a wave stops the scan only when IT has seen more than four values; here every wave sees {0,1,2,3} or {4,5,6,7}
    # (for waves = W; W - 1 and W + 1 shift the pattern, so that the test does not hang on the formula), and the host
    # has to refuse the DNA path from the union
    import kiss_amd
    assert PRESENCE_WAVES_1M == 248
    n = 1_000_000
    rng = np.random.default_rng(waves)
    chunk = np.arange(n) // 64
    S = (rng.integers(0, 4, n) + 4 * ((chunk % waves) % 2)).astype(np.uint8)
    assert np.unique(S).size == 8
    for c in range(0, n // 64, 997):
        assert np.unique(S[64 * c:64 * c + 64] // 4).size == 1
    sa = sort_u8_on(gctx, torch_dev, S)
    assert is_suffix_array(S, sa)
    monkeypatch.setenv("KISS_HIP_NO_SMALL_ALPHABET", "1")  # (a switch of the hooks build)
    assert np.array_equal(kiss_amd.suffix_array_bytes(S, hooks=True), sa)


@pytest.mark.parametrize("where", ["first", "last", 4096])
def test_a_fifth_value_that_occurs_once(gctx, torch_dev, monkeypatch, where):
    import kiss_amd
    n = 1_000_000
    S = np.frombuffer(b"ACGT", np.uint8)[gen.genome_like(n, 5)].copy()
    S[{"first": 0, "last": n - 1}.get(where, where)] = 200
    assert np.unique(S).size == 5
    sa = sort_u8_on(gctx, torch_dev, S)
    assert is_suffix_array(S, sa)
    monkeypatch.setenv("KISS_HIP_NO_SMALL_ALPHABET", "1")
    assert np.array_equal(kiss_amd.suffix_array_bytes(S, hooks=True), sa)


def _deep_tie_text(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind.startswith("unit"):
        unit = rng.integers(0, 256, int(kind[4:]), dtype=np.uint8)
        S = np.tile(unit, n // unit.size + 1)[:n].copy()
        S[rng.choice(n, 8, replace=False)] = rng.choice(256, 8, replace=False).astype(np.uint8)  # a few mutations
    elif kind == "ends_in_its_beginning":
        S = rng.integers(0, 256, n, dtype=np.uint8)
        S[n - n // 3:] = S[:n // 3]
    else:
        assert kind == "equal_runs"
        S = rng.integers(0, 256, n, dtype=np.uint8)
        run = n // 3
        S[n // 10:n // 10 + run] = 77
        S[n // 2:n // 2 + run] = 77
    assert np.unique(S).size > 4  # the 7-character path and its doubling rounds, not the DNA path
    return S


@pytest.mark.parametrize("kind", ["unit1", "unit2", "unit7", "unit8", "unit13", "unit255", "ends_in_its_beginning",
                                  "equal_runs"])
def test_deep_ties_over_more_than_four_values(gctx, torch_dev, kind):
    # ties far deeper than the 7-character key: the doubling rounds from h = 7 do the work (runs of 100 000 equal
    # bytes at n = 300 000)
    for n in (20_000, 300_000):
        S = _deep_tie_text(kind, n, 40 + n % 7)
        check_bytes_sa(S, sort_u8_on(gctx, torch_dev, S))


def test_one_context_through_a_sequence_of_byte_and_dna_calls(torch_dev, oracle):
    # what one call leaves behind must not reach the next: DNA k = 256 -> bytes over 256 values (grows the per-LMS
    # arrays to n items) -> a four-value byte text (allocates the code buffer of the DNA detour) -> a shorter text over
    # 256 values -> DNA k = 256 -> DNA exact; max_n larger than every n
    import kiss_amd
    torch, dev = torch_dev
    rng = np.random.default_rng(6)
    dna = gen.genome_like(500_000, 8)
    with kiss_amd.Context(max_n=1_200_000, device=0) as c:
        def dna_sort(S, k):
            d_S = torch.from_numpy(S).to(dev)
            d_SA = torch.full((S.size + 1,), -1, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            c.suffix_sort_dev(d_S.data_ptr(), S.size, d_SA.data_ptr(), k=k)
            assert c.verify_sa_dev(d_S.data_ptr(), S.size, d_SA.data_ptr(), k)["ok"] == 1
            assert np.array_equal(d_SA.cpu().numpy().view(np.uint32), oracle.suffix_sort(S, k))

        dna_sort(dna, 256)
        S = rng.integers(0, 256, 1_000_000, dtype=np.uint8)
        assert is_suffix_array(S, sort_u8_on(c, torch_dev, S))
        four = np.frombuffer(b"\x07\x40\x80\xff", np.uint8)[gen.genome_like(700_000, 9)]
        sa = sort_u8_on(c, torch_dev, four)
        assert is_suffix_array(four, sa)
        assert np.array_equal(sa, oracle.suffix_sort(gen.genome_like(700_000, 9), K_UNBOUNDED))
        S = rng.integers(0, 256, 250_000, dtype=np.uint8)
        S[200_000:] = S[:50_000]
        check_bytes_sa(S, sort_u8_on(c, torch_dev, S))
        dna_sort(dna, 256)
        dna_sort(dna, K_UNBOUNDED)
