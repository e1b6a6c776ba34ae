"""Pins the oracle (oracle/kiss_oracle.c, our restatement) against the REFERENCE'S OWN CODE compiled unmodified into
oracle/_ref/libkiss_ref.so (oracle/ref_driver.cpp): get_lms, the PackedDNAString loads the comparator is built from,
put_lms_suffix and the induction sweeps.  CPU only.  What stays restated on both sides (the control flow of
lms_suffix_direct_sort_dna, kiss1_core.hpp:41-144 -- that header needs spdlog) is cross-checked between two
independent restatements (C byte compares in the oracle, AVX2 block compares on the reference's packed loads in the
driver).

The reference's outputs on the inputs below are recorded in tests/golden/ref_pin_record.json (FNV-1a-64 of each array,
the histograms and the 10-mer prefixes as they are) and tests/golden/ref_pin_load125.npy (the 256-bit loads) by
tests/golden/make_ref_pin_record.py, where the reference sources are at hand; the tests compare the oracle with that
record, so they run on every box."""
import json
import os

import numpy as np
import pytest

from tests import gen

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RECORD = os.path.join(GOLDEN, "ref_pin_record.json")
LOAD125 = os.path.join(GOLDEN, "ref_pin_load125.npy")

KS = [32, 256, 0xFFFFFFFF]


def shapes():
    yield "iid_100003", gen.iid(100_003, 1)
    yield "iid_20000", gen.iid(20_000, 2)
    yield "genome_300k", gen.genome_like(300_000, 3)
    yield "genome_1M", gen.genome_like(1_000_000, 4)
    for p in (1, 2, 3, 5, 7, 37, 400):
        yield "periodic_%d" % p, gen.periodic(30_000, p, 10 + p, mutations=4)
    yield "all_A", np.zeros(20_000, np.uint8)
    yield "all_T", np.full(12_345, 3, np.uint8)
    yield "AC_n", np.tile(np.array([0, 1], np.uint8), 10_000)
    for cut in (124, 125, 126, 255, 256, 257, 374, 375, 376, 500):
        # text ending inside a repeat: a copy of the head at the very end, cut after `cut` bases (end-of-text rule)
        base = gen.iid(20_000, 50 + cut)
        yield "endrepeat_%d" % cut, np.concatenate([base, base[:cut]])
    for n in (1, 2, 3, 5, 16, 50, 1000):
        yield "tiny_%d" % n, gen.iid(n, 70 + n)


SHAPES = list(shapes())


def prefix10_input():
    S = gen.iid(5000, 5)
    idx = np.concatenate([np.arange(0, 64), np.arange(S.size - 40, S.size + 1)]).astype(np.uint32)
    return S, idx


def load125_input():
    S = gen.periodic(6000, 37, 3, mutations=40)
    idx = np.random.default_rng(1).integers(0, S.size - 125, 400).astype(np.uint32)
    return S, idx


def fnv_hex(oracle, a):
    return "%016x" % oracle.fnv(a)


@pytest.fixture(scope="module")
def ref():
    """what the reference's code returned on these inputs (make_ref_pin_record.py)"""
    with open(RECORD) as f:
        rec = json.load(f)
    rec["load125"] = np.load(LOAD125)
    return rec


@pytest.mark.parametrize("name,S", SHAPES, ids=[s[0] for s in SHAPES])
def test_get_lms_equals_reference(oracle, ref, name, S):
    lms_o, hist_o = oracle.get_lms(S)
    for T in (1, 3, 8):
        r = ref["get_lms"][name][str(T)]
        assert lms_o.size == r["m"] and fnv_hex(oracle, lms_o) == r["lms_fnv"], (name, T)
        # the reference's per-thread buckets summed over the threads (kiss_common.hpp:431-436)
        assert hist_o[:, :4].tolist() == r["hist"], (name, T)


def key_of(S, p, L):
    seg = np.zeros(L, np.uint8)
    part = S[p:p + L]
    seg[:part.size] = part
    return seg


def test_prefix10_load_is_first_10_bases_zero_padded(ref):
    S, idx = prefix10_input()
    got = ref["prefix10"]
    assert len(got) == idx.size
    for p, g in zip(idx.tolist(), got):
        v = 0
        for b in key_of(S, p, 10).tolist():
            v = (v << 2) | b
        assert g == v, p


def test_load125_orders_like_the_first_125_bases(ref):
    # the 256-bit word of load_prefix_length_125 compared most-significant-byte-first (what the comparator does with it,
    # kiss1_core.hpp:103-113) must order positions exactly like their first 125 bases
    S, idx = load125_input()
    words = ref["load125"]
    assert words.shape == (idx.size, 32)
    keys_ref = [bytes(w[::-1]) for w in words]  # byte 31 first
    keys_txt = [S[p:p + 125].tobytes() for p in idx.tolist()]
    for a in range(0, 400, 7):
        for b in range(0, 400, 11):
            assert (keys_ref[a] < keys_ref[b]) == (keys_txt[a] < keys_txt[b])
            assert (keys_ref[a] == keys_ref[b]) == (keys_txt[a] == keys_txt[b])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,S", SHAPES, ids=[s[0] for s in SHAPES])
def test_induction_by_reference_code_only(oracle, ref, name, S, k):
    """LMS order from the oracle, then ONLY reference code: get_lms + put_lms_suffix + induced_sort (multi-threaded
    block scheduling included) -> must reproduce the oracle's SA bit for bit."""
    sa_o, lms_sorted_o = oracle.suffix_sort(S, k, stages=True)
    r = ref["induction"][name][str(k)]
    assert fnv_hex(oracle, lms_sorted_o) == r["lms_sorted_fnv"], (name, k)  # the LMS order the reference code was given
    for T in (1, 4):
        assert fnv_hex(oracle, sa_o) == r["sa_fnv"][str(T)], (name, k, T)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,S", SHAPES, ids=[s[0] for s in SHAPES])
def test_full_pipeline_two_restatements_of_the_comparator_agree(oracle, ref, name, S, k):
    sa_o, lms_o = oracle.suffix_sort(S, k, stages=True)
    r = ref["pipeline"][name][str(k)]
    assert fnv_hex(oracle, lms_o) == r["lms_sorted_fnv"], (name, k)
    assert fnv_hex(oracle, sa_o) == r["sa_fnv"], (name, k)


def test_committed_oracle_goldens_equal_reference(oracle, ref):
    """tests/golden/*.npz were written by the oracle (make_golden.py); the reference's own get_lms / placement /
    induction reproduce every one of them"""
    files = sorted(f for f in os.listdir(GOLDEN) if f.endswith(".npz"))
    assert files and files == sorted(ref["goldens"])
    for f in files:
        z = np.load(os.path.join(GOLDEN, f))
        assert fnv_hex(oracle, z["SA"]) == ref["goldens"][f], f
