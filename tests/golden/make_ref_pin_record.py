#!/usr/bin/env python3
"""Writes tests/golden/ref_pin_record.json and tests/golden/ref_pin_load125.npy: what the REFERENCE'S OWN code
(oracle/_ref/libkiss_ref.so, built by oracle/Makefile from the reference sources; see oracle/ref_driver.cpp for what is
and is not reference code) returns on the inputs of tests/test_ref_pin.py.  Run where those sources are at hand; the
record (data only: FNV-1a-64 of u32-LE arrays, histograms, 10-mer prefixes, 256-bit loads) travels, the reference does not.

  get_lms   : per shape and thread count (1, 3, 8): the ascending LMS list and the first four columns of the histogram
  prefix10  : kref_prefix10 on prefix10_input()
  load125   : kref_load125 on load125_input() (the .npy)
  induction : per shape and k: the oracle's k-ordered LMS list handed to the reference's put_lms_suffix + induced_sort,
              and the suffix array that came back at 1 and 4 threads
  pipeline  : per shape and k: ref_driver.cpp's restated LMS sort + the reference's induction, LMS list and SA
  goldens   : per tests/golden/*.npz written by make_golden.py: the reference pipeline's SA of its text
--check compares a fresh run with the committed record instead of writing it."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import oracle_binding, ref_binding  # noqa: E402
from tests import test_ref_pin as t  # noqa: E402


def record():
    orc, ref = oracle_binding.load(), ref_binding.load()

    def h(a):
        return "%016x" % orc.fnv(a)

    rec = {"made_by": "tests/golden/make_ref_pin_record.py", "get_lms": {}, "induction": {}, "pipeline": {}, "goldens": {}}
    for name, S in t.SHAPES:
        rec["get_lms"][name] = {}
        for T in (1, 3, 8):
            lms, hist = ref.get_lms(S, T)
            rec["get_lms"][name][str(T)] = {"m": int(lms.size), "lms_fnv": h(lms), "hist": hist[:, :4].tolist()}
        rec["induction"][name], rec["pipeline"][name] = {}, {}
        for k in t.KS:
            _, lms_sorted_o = orc.suffix_sort(S, k, stages=True)
            rec["induction"][name][str(k)] = {
                "lms_sorted_fnv": h(lms_sorted_o),
                "sa_fnv": {str(T): h(ref.suffix_sort(S, k, T=T, sorted_lms=lms_sorted_o)) for T in (1, 4)}}
            sa_r, lms_r = ref.suffix_sort(S, k, stages=True)
            rec["pipeline"][name][str(k)] = {"lms_sorted_fnv": h(lms_r), "sa_fnv": h(sa_r)}
        print(name, flush=True)
    S, idx = t.prefix10_input()
    rec["prefix10"] = [int(v) for v in ref.prefix10(S, idx)]
    for f in sorted(os.listdir(t.GOLDEN)):
        if f.endswith(".npz"):
            z = np.load(os.path.join(t.GOLDEN, f))
            rec["goldens"][f] = h(ref.suffix_sort(z["S"], int(z["k"])))
    S, idx = t.load125_input()
    return rec, ref.load125(S, idx)


if __name__ == "__main__":
    rec, words = record()
    if "--check" in sys.argv[1:]:
        with open(t.RECORD) as f:
            old = json.load(f)
        same = old == json.loads(json.dumps(rec)) and np.array_equal(np.load(t.LOAD125), words)
        print("record matches the reference" if same else "record DIFFERS from the reference")
        sys.exit(0 if same else 1)
    with open(t.RECORD, "w") as f:
        json.dump(rec, f, indent=1)
    np.save(t.LOAD125, words)
    print("wrote", t.RECORD, t.LOAD125)
