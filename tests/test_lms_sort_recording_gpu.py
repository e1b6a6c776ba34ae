"""Which steps the LMS sort and the two rank-doubling forms run, over how many items: a recording (kiss_amd/csrc/lms_sort.hip,
doubling.hip, flag_compact.hip).

tests/golden/lms_sort_recording.json holds, for every case below, the counters of kiss_hip_get_stats that say which steps
ran -- lms_rounds, sort_item_rounds, pair_records, big_item_rounds, doubling_rounds, refine_items, refine_form, the depths
-- and the launch and item counts of all sixteen kernel classes (every KTimer scope counts when all classes are profiled),
plus the FNV of the suffix array.  A change that is meant to move code and nothing else must leave every figure as it is.
The file is written by record() (python -m tests.test_lms_sort_recording_gpu, on the GPU) and never by a test; the suffix
array's FNV must also be the oracle's, at recording time and in the test.

Cases: the texts of test_small_segments_gpu plus two -- `all_tied`, (AC)^n with n = 2^18 (every LMS suffix tied with every
other one at any bounded depth; with KISS_HIP_TCAP0=1024 both regrow paths of round 0 run), and `one_segment`, one random
3000-base unit repeated to 300 000 bases (a single huge tied segment per phase of the unit: segment ids of no bits, and in
exact order the 32-base rounds give up and both doubling forms run) -- in the four modes of that file, with the shipped
library, and for four of the texts with the hooks library and exactly one switch each.
"""
import json
import os
import sys

import numpy as np
import pytest

from tests.test_small_segments_gpu import K_UNBOUNDED, MODES, ONEPASS_MIN, _texts

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lms_sort_recording.json")
SCALARS = ("lms_rounds", "sort_item_rounds", "pair_records", "big_item_rounds", "doubling_rounds", "refine_items",
           "refine_form", "depth", "refine_depth")
# one switch of the hooks build per case ("" = none)
SWITCHES = [("", ""), ("KISS_HIP_NO_FC0_ONEPASS", "1"), ("KISS_HIP_NO_PAIR_RECORDS", "1"), ("KISS_HIP_NO_SMALL_FUSED", "1"),
            ("KISS_HIP_NO_PIVOT_ROUNDS", "1"), ("KISS_HIP_PIVOT_FROM_ROUND2", "1"), ("KISS_HIP_PIVOT_SLOTS", "1"),
            ("KISS_HIP_NO_PIVOT_CTX", "1"), ("KISS_HIP_PAIR_KEYS", "1"), ("KISS_HIP_NO_LMS_EXACT", "1"),
            ("KISS_HIP_LMS_HEADS_BY_COMPARE", "1"), ("KISS_HIP_NO_TAINT", "1"), ("KISS_HIP_TCAP0", "1024")]
EXACT_ONLY = ("KISS_HIP_NO_LMS_EXACT", "KISS_HIP_LMS_HEADS_BY_COMPARE", "KISS_HIP_NO_TAINT", "KISS_HIP_TCAP0")
HOOK_TEXTS = ("genome_like", "mixed_small", "all_tied", "one_segment")
TWO_PASS_TEXTS = ("tiny_triples", "one_block_triples")  # fewer than 8 tiles of round-0 items


def _all_texts():
    t = _texts()
    t["all_tied"] = np.tile(np.array([0, 1], np.uint8), 1 << 18)
    t["one_segment"] = np.tile(np.random.default_rng(12).integers(0, 4, 3000, dtype=np.uint8), 100)
    return t


TEXT_NAMES = ("genome_like", "mixed_small", "one_block_triples", "short_arrays", "tiny_triples", "triples_exact", "all_tied",
              "one_segment")


def _cases():
    """case id -> (text, k, algo, hooks library?, switch, value)"""
    cases = {}
    for name in TEXT_NAMES:
        for k, algo in MODES:
            mode = "k%s-algo%d" % ("inf" if k == K_UNBOUNDED else str(k), algo)
            cases["%s-%s-shipped" % (name, mode)] = (name, k, algo, False, "", "")
            if name not in HOOK_TEXTS:
                continue
            for switch, value in SWITCHES:
                if switch in EXACT_ONLY and k != K_UNBOUNDED:
                    continue  # the exact-order finish, or a regrow that only all-tied exact rounds reach
                what = (switch[len("KISS_HIP_"):].lower() + ("=" + value if value != "1" else "")) if switch else "hooks"
                cases["%s-%s-%s" % (name, mode, what)] = (name, k, algo, True, switch, value)
    return cases


CASES = _cases()


def _run(case, texts, oracle):
    """one sort in a context of its own -> (the recorded figures, the suffix array's FNV)"""
    import kiss_amd
    name, k, algo, hooks, switch, value = CASES[case]
    S = texts[name]
    for sw, _ in SWITCHES:
        if sw:
            assert sw not in os.environ, sw
    if switch:
        os.environ[switch] = value
    try:
        with kiss_amd.Context(max_n=S.size, device=0, profiling=True, hooks=hooks) as c:
            sa = c.suffix_sort(S, k, algo=algo)
            st = c.stats()
    finally:
        if switch:
            del os.environ[switch]
    got = {key: int(st[key]) for key in SCALARS}
    got["launches_kernel"] = [int(st["kernels"][kc]["launches"]) for kc in kiss_amd._lib.KERNEL_CLASSES]
    got["items_kernel"] = [int(st["kernels"][kc]["items"]) for kc in kiss_amd._lib.KERNEL_CLASSES]
    got["sa_fnv"] = "%016x" % oracle.fnv(sa)
    return got


@pytest.fixture(scope="module")
def texts():
    return _all_texts()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {"cases": {case: dict(zip(g["fields"], row)) for case, row in g["cases"].items()}}


@pytest.fixture(scope="module")
def oracle_fnv(texts, oracle):
    """(text, k) -> FNV of the oracle's suffix array, computed once.  The oracle's comparison sort needs half a minute for
    the exact order of (AC)^n; there the test takes the closed form of that (unique) suffix array, which record() holds
    against the oracle's."""
    cache = {}

    def get(name, k):
        if (name, k) not in cache:
            sa = _exact_sa_of_all_tied(texts[name].size) if (name, k) == ("all_tied", K_UNBOUNDED) else oracle.suffix_sort(texts[name], k)
            cache[(name, k)] = "%016x" % oracle.fnv(sa)
        return cache[(name, k)]
    return get


def _exact_sa_of_all_tied(n):
    """(AC)^(n/2): a suffix is a prefix of every longer suffix that starts with the same base, so the shorter one sorts
    first -- the sentinel, the suffixes at even positions from the end, the suffixes at odd positions from the end"""
    return np.concatenate([[n], np.arange(n - 2, -1, -2), np.arange(n - 1, 0, -2)]).astype(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_sort_runs_the_recorded_steps(case, texts, golden, oracle, oracle_fnv):
    got = _run(case, texts, oracle)
    want = golden["cases"][case]
    for key in sorted(want):
        assert got[key] == want[key], (case, key, got[key], want[key])
    assert got["sa_fnv"] == oracle_fnv(CASES[case][0], CASES[case][1]), case


def test_the_recording_has_every_case_and_reaches_every_path(golden):
    rec = golden["cases"]
    assert sorted(rec) == sorted(CASES)
    for want in rec.values():
        assert sorted(want) == sorted(FIELDS)
        assert len(want["launches_kernel"]) == 16 and len(want["items_kernel"]) == 16
    assert any(r["pair_records"] > 0 for r in rec.values())
    assert any(r["big_item_rounds"] > 0 for r in rec.values())
    assert any(r["doubling_rounds"] > 0 and r["refine_form"] == 1 for r in rec.values())
    assert any(r["doubling_rounds"] > 0 and r["refine_form"] == 2 for r in rec.values())
    assert any(r["lms_rounds"] > 9 for r in rec.values())  # the 32-base rounds ran
    # one result per (text, k), whatever the form
    for case, (name, k, algo, hooks, switch, value) in CASES.items():
        assert rec[case]["sa_fnv"] == rec["%s-k%s-algo0-shipped" % (name, "inf" if k == K_UNBOUNDED else str(k))]["sa_fnv"], case


def test_the_texts_reach_the_round0_form_they_are_meant_for(texts, golden, oracle):
    """the one-pass round 0 needs 8 tiles of 8192 far LMS suffixes; the two tiny texts must stay below that"""
    for name in TEXT_NAMES:
        S = texts[name]
        lms = oracle.get_lms(S)[0][:-1].astype(np.int64)
        for k, algo in MODES:
            st = golden["cases"]["%s-k%s-algo%d-shipped" % (name, "inf" if k == K_UNBOUNDED else str(k), algo)]
            depth = 125 * (st["refine_depth"] // 125 + 1) if st["refine_depth"] else st["depth"]
            m_far = int(np.sum(lms + depth <= S.size)) if depth else lms.size
            if name in TWO_PASS_TEXTS:
                assert m_far < ONEPASS_MIN, (name, k, algo, m_far)
            else:
                assert m_far > ONEPASS_MIN, (name, k, algo, m_far)  # (>= 8 full tiles + 1: ceil(m_far / 8192) >= 8 needs 57 345)


FIELDS = SCALARS + ("launches_kernel", "items_kernel", "sa_fnv")


def _write(cases, path):
    """the golden file: the field names once, then one case per line with its values in that order"""
    rows = ['"%s":%s' % (case, json.dumps([cases[case][f] for f in FIELDS], separators=(",", ":"))) for case in sorted(cases)]
    with open(path, "w") as f:
        f.write('{"fields":%s,\n"cases":{\n' % json.dumps(list(FIELDS)) + ",\n".join(rows) + "\n}}\n")


def record(path=GOLDEN):
    """runs every case on the GPU and writes the golden file; every suffix array must be the oracle's"""
    from tests import oracle_binding
    oracle = oracle_binding.load()
    texts = _all_texts()
    want_fnv = {}
    out = {}
    for case in sorted(CASES):
        name, k = CASES[case][0], CASES[case][1]
        if (name, k) not in want_fnv:
            want_fnv[(name, k)] = "%016x" % oracle.fnv(oracle.suffix_sort(texts[name], k))
            if (name, k) == ("all_tied", K_UNBOUNDED):
                assert want_fnv[(name, k)] == "%016x" % oracle.fnv(_exact_sa_of_all_tied(texts[name].size))
        out[case] = _run(case, texts, oracle)
        assert out[case]["sa_fnv"] == want_fnv[(name, k)], case
        print(case, json.dumps(out[case]), flush=True)
    _write(out, path)


if __name__ == "__main__":
    record(*sys.argv[1:2])
