"""Record sets for the duplicate-marking tests (tests/test_markdup_model.py, tests/test_markdup_gpu.py): templates built with
tests/markdup_model.record, whose ends are drawn from few places so that they collide."""
import numpy as np

from tests import markdup_model as M


def quals(rng, n, lo=10, hi=20):
    return bytes(rng.integers(lo, hi + 1, n, dtype=np.uint8))


def mapped(name, flag, ref, pos, rng, reverse=False, lead=0, trail=0, match=20, hard=False, qual=None, flat=False):
    """a mapped record of `match` aligned bases with clips of `lead` and `trail` bases around them (hard: H clips, which hold no
    bases; flat: every quality is 30, so that scores tie)"""
    cigar = ([(lead, "H" if hard else "S")] if lead else []) + [(match, "M")] + ([(trail, "H" if hard else "S")] if trail else [])
    L = match + (0 if hard else lead + trail)
    return M.record(name, flag | (16 if reverse else 0), ref, pos, cigar, (b"\x1e" * L if flat else quals(rng, L)) if qual is None else qual)


def unmapped(name, flag, rng, ref=-1, pos=-1, n=20):
    return M.record(name, flag | 4, ref, pos, (), quals(rng, n))


def pair(name, rng, ref, pos1, pos2, rev1=False, rev2=True, swap=False, **how):
    """the two primaries of a pair; swap: the second mate stands first in the file"""
    a = mapped(name, 0x41, ref, pos1, rng, rev1, **how)
    b = mapped(name, 0x81, ref, pos2, rng, rev2, **how)
    return [b, a] if swap else [a, b]


def random_set(rng, templates, n_ref=3, places=(100, 101, 130, 5000), names=None):
    """`templates` templates of every class with colliding ends -> the list of records"""
    out = []
    for t in range(templates):
        name = b"t%d" % t if names is None else names[t]
        ref = int(rng.integers(0, n_ref))
        p1, p2 = int(rng.choice(places)), int(rng.choice(places))
        kind = int(rng.integers(0, 10))
        clip = dict(lead=int(rng.integers(0, 3)), trail=int(rng.integers(0, 3)), hard=bool(rng.integers(0, 2)), flat=bool(rng.integers(0, 2)))
        if kind <= 3:
            recs = pair(name, rng, ref, p1, p2, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), **clip)
            if rng.integers(0, 4) == 0:  # a supplementary and a secondary record of the first mate
                recs.insert(1, mapped(name, 0x841, ref, 7, rng))
                recs.append(mapped(name, 0x141, ref, 9, rng))
            if rng.integers(0, 8) == 0:
                recs[0] = recs[0][:18] + bytes([recs[0][18], recs[0][19] | 4]) + recs[0][20:]  # a stale 0x400
        elif kind <= 6:
            recs = [mapped(name, int(rng.choice([0, 0x41, 0x81])), ref, p1, rng, bool(rng.integers(0, 2)), **clip)]
            if rng.integers(0, 3) == 0:
                recs.append(mapped(name, 0x100, ref, 11, rng))
        elif kind == 7:  # a mapped mate and an unmapped one, placed at its partner
            recs = [mapped(name, 0x49, ref, p1, rng, bool(rng.integers(0, 2)), **clip), unmapped(name, 0x85, rng, ref, p1)]
            if rng.integers(0, 2):
                recs.reverse()
        elif kind == 8:
            recs = [unmapped(name, 0, rng)] if rng.integers(0, 2) else [unmapped(name, 0x4D, rng), unmapped(name, 0x8D, rng)]
        else:  # ambiguous: two single-end reads of one name; two first mates; three primaries
            which = int(rng.integers(0, 3))
            if which == 0:
                recs = [mapped(name, 0, ref, p1, rng), mapped(name, 0, ref, p2, rng)]
            elif which == 1:
                recs = [mapped(name, 0x41, ref, p1, rng), mapped(name, 0x41, ref, p2, rng)]
            else:
                recs = pair(name, rng, ref, p1, p2) + [mapped(name, 0x81, ref, p2, rng)]
        out += recs
    return out
