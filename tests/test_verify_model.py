"""The host model of the device verifier (tests/verify_model.py) and the mutation generators (tests/verify_mutations.py),
checked where there is no GPU: the model against the oracle's suffix arrays, its digest against the library's host
helper, every generator against the verdict its docstring promises, and the share conditions of the randomised block."""
import numpy as np
import pytest

from tests import gen, verify_model, verify_mutations as vm
from tests.test_suffix_sort_gpu import _random_text

K_UNBOUNDED = verify_model.K_UNBOUNDED


def _shape(name):
    return {"iid": lambda: gen.iid(200_003, 1), "genome": lambda: gen.genome_like(1_000_000, 2),
            "period3": lambda: gen.periodic(50_000, 3, 3, 5), "period171": lambda: gen.periodic(80_000, 171, 4, 50),
            "allA": lambda: np.zeros(10_000, np.uint8), "tiny0": lambda: np.zeros(0, np.uint8),
            "tiny1": lambda: gen.iid(1, 5), "tiny9": lambda: gen.iid(9, 6)}[name]()


@pytest.mark.parametrize("shape", ["iid", "genome", "period3", "period171", "allA", "tiny0", "tiny1", "tiny9"])
def test_model_accepts_the_oracles_suffix_arrays(oracle, shape):
    S = _shape(shape)
    n = S.size
    for k in (1, 8, 32, 256, K_UNBOUNDED):
        SA = oracle.suffix_sort(S, k)
        if k < n and n > 300_000:  # (Python byte compares: the full bounded model stays at n <= 300 000)
            rep = verify_model.report_near(S, SA, k, range(0, n + 1, 7))
        else:
            rep = verify_model.report(S, SA, k)
        assert rep["ok"] == 1 and rep["order_violations"] == 0 and rep["first_violation"] == 0, (k, rep)
        assert (rep["sa0_ok"], rep["duplicates"], rep["out_of_range"]) == (1, 0, 0), (k, rep)
        assert rep["exact"] == (1 if k >= n else 0)
        if k >= n:
            assert rep["tied_pairs"] == 0 and verify_model.is_suffix_array(S, SA)
    if shape == "allA":  # every pair of full-length substrings is tied: n - k of them
        assert verify_model.report(S, oracle.suffix_sort(S, 32), 32)["tied_pairs"] == n - 32


def test_model_rejects_a_k_ordered_array_in_exact_mode(oracle):
    S = gen.genome_like(300_000, 7)
    SA, exact = oracle.suffix_sort(S, 256), oracle.suffix_sort(S, K_UNBOUNDED)
    assert not np.array_equal(SA, exact)
    rep = verify_model.report(S, SA, K_UNBOUNDED)
    assert rep["exact"] == 1 and rep["ok"] == 0 and rep["order_violations"] > 0 and rep["first_violation"] >= 1
    assert (rep["sa0_ok"], rep["duplicates"], rep["out_of_range"]) == (1, 0, 0)
    assert not verify_model.is_suffix_array(S, SA) and verify_model.is_suffix_array(S, exact)
    assert verify_model.report(S, SA, 256)["ok"] == 1


def test_exact_model_against_sorted_python_suffixes():
    rng = np.random.default_rng(3)
    for case in range(200):
        n = int(rng.integers(0, 40))
        S = rng.integers(0, int(rng.choice([1, 2, 4, 256])), n, dtype=np.uint8)
        SA = vm.naive_sa(S)
        assert verify_model.is_suffix_array(S, SA)
        if n >= 2:  # any other permutation with the sentinel first is not the suffix array
            other = SA.copy()
            other[1:] = rng.permutation(SA[1:])
            assert verify_model.is_suffix_array(S, other) == np.array_equal(other, SA)
            rep = verify_model.report(S, other, K_UNBOUNDED)
            assert rep["ok"] == (1 if np.array_equal(other, SA) else 0)
            # bounded model against the definition, pair by pair
            k = int(rng.integers(1, n))
            b = S.tobytes()
            viol = [i for i in range(1, n + 1) if b[other[i - 1]:other[i - 1] + k] > b[other[i]:other[i] + k]]
            rep = verify_model.report(S, other, k)
            assert rep["order_violations"] == len(viol) and rep["first_violation"] == (viol[0] if viol else 0)


@pytest.mark.parametrize("count", [0, 1, 2, 1000, 100_003])
def test_model_digest_equals_the_host_helper(count):
    from kiss_amd import sorter
    rng = np.random.default_rng(count)
    for _ in range(3):
        SA = rng.integers(0, 1 << 32, count, dtype=np.uint64).astype(np.uint32)
        assert verify_model.digest(SA) == sorter.sa_digest(SA)
    perm = rng.permutation(count).astype(np.uint32)
    assert verify_model.digest(perm) == sorter.sa_digest(perm)
    if count >= 2:  # order-sensitive
        assert verify_model.digest(perm) != verify_model.digest(perm[::-1].copy())


def test_digest_in_python_integers():
    # the formula once more, in unbounded Python integers reduced modulo 2^64
    M = (1 << 64) - 1
    SA = [5, 0, 0xFFFFFFFF, 7, 123456789]
    total = 0
    for i, v in enumerate(SA):
        x = ((i << 32) ^ v ^ (0x5851F42D4C957F2D * i & M)) & M
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        total = (total + (x ^ (x >> 31))) & M
    assert verify_model.digest(np.array(SA, np.uint32)) == total


@pytest.mark.parametrize("family", vm.FAMILIES)
def test_every_generator_gives_the_verdict_it_promises(oracle, family):
    count = 0
    for label, case in vm.cases(family, oracle.suffix_sort, _random_text):
        rep = verify_model.report(case.S, case.SA, case.k)
        for field, value in case.what_must_hold.items():
            assert rep[field] is None or rep[field] == value, (family, label, field, value, rep)
        if case.k < case.S.size:  # the near form sees what the full form sees
            near = verify_model.report_near(case.S, case.SA, case.k, case.touched)
            for field in ("ok", "order_violations", "first_violation", "duplicates", "out_of_range", "sa0_ok", "digest"):
                assert near[field] == rep[field], (family, label, field, near, rep)
        count += 1
    assert count >= 50, (family, count)


def test_undefined_fields_are_not_stated():
    S = gen.iid(500, 1)
    SA = vm.naive_sa(S)
    dup = vm.duplicate_values(S, SA, K_UNBOUNDED, 3, [9])
    rep = verify_model.report(dup.S, dup.SA, dup.k)
    assert rep["order_violations"] is None and rep["first_violation"] is None and rep["ok"] == 0
    assert "order_violations" not in verify_model.comparable(rep) and "duplicates" in verify_model.comparable(rep)
    rep = verify_model.report(dup.S, dup.SA, 32)  # bounded k needs no ranks: every field is stated
    assert verify_model.comparable(rep) == list(verify_model.FIELDS)


def test_randomised_block_meets_its_shares(oracle):
    models = []
    for block in range(vm.RANDOM_BLOCKS):
        rng = np.random.default_rng(vm.RANDOM_SEED + block)
        for _ in range(vm.RANDOM_CASES_PER_BLOCK):
            case = vm.random_case(rng, oracle.suffix_sort, _random_text)
            models.append(verify_model.report(case.S, case.SA, case.k))
    vm.check_shares(vm.shares(models))
