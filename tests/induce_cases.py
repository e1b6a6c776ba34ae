"""The model's side of the induction path tests (no GPU): the forced configurations, the grid of (text, k, configuration,
claim) rows, the per-text reference data and the premises each row asserts before anything runs on a device.
tests/test_induce_paths_gpu.py runs the rows; tests/test_induce_model.py checks every row's premises on the CPU."""
import numpy as np

from tests import induce_model as im

K_EXACT = 0xFFFFFFFF
SMALL_MAX, COLLAPSE_N = 8192, 1 << 18          # shipped thresholds (induce.hip)
ROOMY_N = 6_000_000                            # a context this large never limits the collapse step by its capacity

SWITCHES = ("KISS_HIP_INDUCE_SMALL_MAX", "KISS_HIP_COLLAPSE_N", "KISS_HIP_COLLAPSE_CAP", "KISS_HIP_NO_CLASS_BYTES",
            "KISS_HIP_INDUCE_ONE_PASS", "KISS_HIP_MERGE_LMS", "KISS_HIP_NO_LMS_EXACT")
_TILES = {"KISS_HIP_INDUCE_SMALL_MAX": 64, "KISS_HIP_COLLAPSE_N": 1024}   # the smallest values the library accepts
CONFIGS = {
    "shipped": {},
    "tiles": dict(_TILES),
    "tiles_words": dict(_TILES, KISS_HIP_NO_CLASS_BYTES=1),
    "tiles_onepass": dict(_TILES, KISS_HIP_INDUCE_ONE_PASS=1),
    "tiles_merged": dict(_TILES, KISS_HIP_MERGE_LMS=1),
    "small_chain": {"KISS_HIP_COLLAPSE_N": 1024},
    "cap1": dict(_TILES, KISS_HIP_COLLAPSE_CAP=1),
    "cap2": dict(_TILES, KISS_HIP_COLLAPSE_CAP=2),
    "cap3": dict(_TILES, KISS_HIP_COLLAPSE_CAP=3),
    "cap7": dict(_TILES, KISS_HIP_COLLAPSE_CAP=7),
    "cap_words": {"KISS_HIP_COLLAPSE_CAP": 3, "KISS_HIP_NO_CLASS_BYTES": 1},
}


def thresholds(config):
    c = CONFIGS[config]
    return c.get("KISS_HIP_INDUCE_SMALL_MAX", SMALL_MAX), c.get("KISS_HIP_COLLAPSE_N", COLLAPSE_N), c.get("KISS_HIP_COLLAPSE_CAP", 0)


# ---- the model's side of a case (no GPU: tests/test_induce_model.py runs plan() for every row of the grids below) -------

class Case:
    pass


_cases = {}


def case_of(oracle, name, k, S=None):
    """text, oracle SA and LMS order, model types / near-end split / schedule / SA -- computed once per (text, k)"""
    key = (name, k)
    if key not in _cases:
        c = Case()
        c.name, c.k = name, k
        c.S = np.ascontiguousarray(im.texts()[name][0]() if S is None else S, dtype=np.uint8)
        c.n = c.S.size
        c.sa_oracle, lms_sorted = oracle.suffix_sort(c.S, k, stages=True)
        c.order = lms_sorted[1:].astype(np.int64)            # the merged k-ordered list without the sentinel
        c.stype, c.lms, c.counts12 = im.types(c.S)
        far_asc, c.near = im.split_near(c.S, c.lms, k)
        isfar = np.zeros(c.n + 1, dtype=bool)
        isfar[far_asc] = True
        c.far_asc = far_asc
        c.far = c.order[isfar[c.order]]                      # the oracle's order filtered to the far positions
        c.sch = im.schedule(c.S, c.order)
        c.want = im.induce(c.S, c.order)
        _cases[key] = c
    return _cases[key]


def forget(name, k):
    _cases.pop((name, k), None)


def forget_all():
    _cases.clear()


def plan(case, config, claim=None, max_n=ROOMY_N):
    """-> the routing (induce_model.Routing) the model expects under `config` on a fresh context for texts up to max_n,
    after asserting what the row claims about the text"""
    small_max, collapse_n, cap = thresholds(config)
    sch = case.sch
    m_cap = im.default_m_cap(max_n)
    assert len(case.lms) <= m_cap, "%s: more LMS suffixes than a fresh context holds, its arrays would regrow" % case.name
    r = im.expected_paths(sch, small_max, collapse_n, m_cap, cap)
    rounds = [N for c in sch.chains.values() for N in c]
    what = "%s under %s" % (case.name, config)
    if claim == "tile_chain":        # count / scan / scatter with a self class, in both directions
        for sweep in "LS":
            assert any(c and c[0] > max(small_max, collapse_n) for (s, b), c in sch.chains.items() if s == sweep), \
                "%s: no %s-sweep chain round goes through the tile kernels" % (what, sweep)
    if claim == "small_chain":       # k_induce_small with selfclass >= 0 chases rounds
        assert any(collapse_n < N <= small_max for N in rounds), "%s: no chain round with %d < N <= %d" % (what, collapse_n, small_max)
        assert r.chased > 0, "%s: the one-workgroup kernel has no further round to chase" % what
    if claim == "cap":               # the closed form continues from its last block at least twice, at the forced cap
        assert cap >= 1 and any(left >= 3 * cap and steps[:3] == [cap] * 3 for key, N, left, steps in r.steps), \
            "%s: no chain takes three closed-form calls of %d steps: %s" % (what, cap, r.steps)
    if claim == "wave_wide":         # several runs longer than RUN_SERIAL (1024) in one round, one of them from position 0
        runs = im.run_lengths(case.S)
        assert sum(1 for a, ln, c in runs if ln > 1024 + 32) >= 8 and runs[0][1] > 1024 + 32, what
        assert any(steps[0] > 1024 + 32 for key, N, left, steps in r.steps), what
    if claim == "wide":              # a first call at the narrow field's limit (not at a capacity limit), then a wide one
        assert max(ln for a, ln, c in im.run_lengths(case.S)) > im.COLLAPSE_RCAP
        for sweep in "LS":
            assert any(key[0] == sweep and m_cap // N >= im.COLLAPSE_RCAP and left > im.COLLAPSE_RCAP
                       and steps[0] == im.COLLAPSE_RCAP and len(steps) >= 2 and steps[1] > im.COLLAPSE_RCAP
                       for key, N, left, steps in r.steps), \
                "%s: no %s chain whose second closed-form call is a wide one: %s" % (what, sweep, r.steps)
    if claim == "capacity":          # m_cap / N, not the field width or a hook, limits the steps, and the chain goes on
        assert cap == 0 and any(steps[0] == m_cap // N < min(left, im.COLLAPSE_RCAP) and len(steps) >= 2 for key, N, left, steps in r.steps), \
            "%s: no closed-form call is limited by m_cap = %d: %s" % (what, m_cap, r.steps)
    return r


# ---- 1-3: random, repetitive and planted-run texts under every configuration ----------------------------------------------
MAIN = [("iid40k", 256), ("genome60k", 256), ("repeat17", 256), ("repeat40", 256), ("planted", 256)]
GRID = [(n, k, c, None) for c in ("shipped", "tiles_words", "tiles_onepass", "tiles_merged") for n, k in MAIN]
GRID += [(n, k, "tiles", "tile_chain" if n in ("iid40k", "genome60k", "planted") else None) for n, k in MAIN]
GRID += [(n, 32, c, None) for n in ("iid40k", "genome60k") for c in ("shipped", "tiles")]
GRID += [(n, 256, "small_chain", "small_chain") for n in ("iid40k", "planted", "planted_short")]
GRID += [(n, 256, c, "cap") for c in ("cap1", "cap2") for n in ("iid40k", "repeat17", "repeat40", "planted_short")]
GRID += [(n, 256, c, "cap") for c in ("cap3", "cap7", "cap_words") for n in ("repeat17", "repeat40", "planted_short")]
# 4: run staircases (rounds of a few items that last 1500 steps); shipped thresholds take them to the closed form, whose run
#    counting goes wave-wide past 1024 bases -- several lanes at once, one of them down to position 0
GRID += [(n, 256, "shipped", "wave_wide") for n in ("stairs_T", "stairs_A")]
GRID += [(n, 256, c, None) for n in ("stairs_T", "stairs_A") for c in ("tiles", "tiles_words", "small_chain", "cap_words")]
GRID += [(n, 256, c, "cap") for n in ("stairs_T", "stairs_A") for c in ("cap3", "cap7")]
# 6, 7: no LMS suffix at all; empty buckets and empty LMS buckets; m = n / 2
GRID += [(n, 256, c, None) for n in ("blocks", "blocks_rev", "AT", "CG", "AC", "ACAC", "TATA") for c in ("shipped", "tiles")]
# 8: tile edges -- the one-workgroup kernel against the tile path at both thresholds, one tile +- 1, four tiles +- 1
GRID += [("edge%d" % x, 32, "tiles", None) for x in (64, 65, 2047, 2048, 2049, 8191, 8192, 8193)]
GRID += [("edge%d" % x, 32, "shipped", None) for x in (8191, 8192, 8193)]
# 9: the near-end table (LmsRemap) with E entries; merged: the same results without the table
GRID += [("near%d" % E, im.NEAR_K, c, None) for E in im.NEAR_E for c in ("shipped", "tiles", "tiles_merged")]



# the forms of the input (context words, shuffled order) run on texts 1-3
FORM_TEXTS = {"shipped": MAIN + [("iid40k", 32), ("genome60k", 32)], "tiles": MAIN + [("iid40k", 32), ("genome60k", 32)],
              "cap3": MAIN[:4] + [("planted_short", 256), ("iid40k", 32), ("genome60k", 32)]}
TIGHT = [(n, c) for n in ("planted", "stairs_T", "iid40k") for c in ("shipped", "tiles")]
