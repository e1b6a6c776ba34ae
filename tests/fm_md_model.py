"""A plain restatement of the MD strings of alignments (include/kiss_hip_md.h, kiss_hip_fmi_md_dev).

md_of() walks one item exactly as the definition reads, column by column; md() runs a batch the way the C call sees it.
rebuild_text() is the inverse that a reader of a SAM line applies: the text under an alignment from the read, the ops and the MD
string alone.  tests/test_fm_md_model.py holds the two against each other and against statements that share neither loop.
"""
import bisect
import re

import numpy as np

from .fm_align_model import virtual_read

LETTERS = "ACGTN"
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*\Z")


def letter(c):
    return LETTERS[min(int(c), 4)]


def is_bad(rec, ops, L, n):
    """rec: (rbeg, rend, tbeg, tend); ops: [(op, len)] -- not empty"""
    rbeg, rend, tbeg, tend = [int(x) for x in rec]
    if any(op > 2 or ln == 0 for op, ln in ops):
        return True
    if sum(ln for op, ln in ops if op in (0, 1)) != rend - rbeg:
        return True
    if sum(ln for op, ln in ops if op in (0, 2)) != tend - tbeg:
        return True
    return rend > L or tend > n or rbeg > rend or tbeg > tend


def md_of(S, Rv, rbeg, tbeg, ops):
    """the walk of one good item -> (string, mismatch columns, deleted bases)"""
    i, j, run = int(rbeg), int(tbeg), 0
    out = []
    mism = dele = 0
    for op, ln in ops:
        if op == 0:
            for _ in range(ln):
                if int(Rv[i]) <= 3 and int(Rv[i]) == int(S[j]):
                    run += 1
                else:
                    out.append("%d%s" % (run, letter(S[j])))
                    run = 0
                    mism += 1
                i, j = i + 1, j + 1
        elif op == 1:
            i += ln
        else:
            out.append("%d^%s" % (run, "".join(letter(c) for c in S[j:j + ln])))
            run = 0
            j += ln
            dele += ln
    out.append("%d" % run)
    return "".join(out), mism, dele


def unpack_ops(words):
    return [(int(w) & 15, int(w) >> 4) for w in words]


def read_of(a, chain_index, both_strands):
    """the largest virtual read v with chain_index[v] <= chain_index[0] + a"""
    x = int(chain_index[0]) + a
    return bisect.bisect_right([int(c) for c in chain_index[:-1]], x) - 1  # (chain_index[0] <= x)


def md(text, reads, alns, chain_index, cigar, cigar_index, both_strands=False, hits=None):
    """a batch as the C call sees it.  alns: rows whose columns 2..5 are rbeg, rend, tbeg, tend (12 columns, the record) or
    a structured array; hits: the aln of every hit, or None -> dict(strings, md (bytes), md_index, md_counts, report counts)"""
    alns = np.asarray(alns)
    if alns.dtype.names:
        quads = np.stack([alns[k].astype(np.int64) for k in ("rbeg", "rend", "tbeg", "tend")], axis=1).reshape(-1, 4)
    else:
        quads = np.asarray(alns, np.int64).reshape(-1, 12)[:, 2:6]
    cidx = [int(c) for c in chain_index]
    V = len(cidx) - 1
    assert V == (2 * len(reads) if both_strands else len(reads))
    C = cidx[V] - cidx[0]
    items = list(range(C)) if hits is None else [int(a) for a in hits]
    n = len(text)
    vreads = {}
    strings, counts, bad = [], [], 0
    for a in items:
        if a >= C:
            bad += 1
            strings.append("")
            counts.append((0, 0))
            continue
        ops = unpack_ops(cigar[int(cigar_index[a]):int(cigar_index[a + 1])])
        if not ops:
            strings.append("")
            counts.append((0, 0))
            continue
        v = bisect.bisect_right(cidx, cidx[0] + a, 0, V) - 1  # (read_of, on the list at hand)
        if v not in vreads:
            vreads[v] = virtual_read(reads[v // 2] if both_strands else reads[v], both_strands and v % 2 == 1)
        Rv = vreads[v]
        if is_bad(quads[a], ops, len(Rv), n):
            bad += 1
            strings.append("")
            counts.append((0, 0))
            continue
        s, mism, dele = md_of(text, Rv, quads[a][0], quads[a][2], ops)
        strings.append(s)
        counts.append((mism, dele))
    index = np.zeros(len(items) + 1, np.uint64)
    np.cumsum([len(s) for s in strings], out=index[1:])
    cnt = np.array(counts, np.uint32).reshape(len(items), 2)
    return {"strings": strings, "md": "".join(strings).encode(), "md_index": index, "md_counts": cnt, "items": len(items), "bad": bad,
            "md_bytes": int(index[-1]), "mismatch_columns": int(cnt[:, 0].sum()), "deleted_bases": int(cnt[:, 1].sum()),
            "longest": max([len(s) for s in strings], default=0)}


def parse_md(s):
    """'10A5^AC6' -> [10, 'A', 5, '^AC', 6]"""
    assert MD_RE.match(s), s
    return [int(t) if t[0].isdigit() else t for t in re.findall(r"[0-9]+|\^[A-Z]+|[A-Z]", s)]


def rebuild_text(Rv, rbeg, ops, md_string):
    """the text under an alignment as letters, from the virtual read, the ops and the MD string alone (no text): M columns take
    the read's base where the string counts a match and the string's letter elsewhere, D ops take the letters behind '^'"""
    toks = parse_md(md_string)
    t = 0          # the token being consumed
    left = toks[0]  # matches left in the current number
    i = int(rbeg)
    out = []

    def next_number():
        nonlocal t, left
        t += 1
        assert isinstance(toks[t], int)
        left = toks[t]

    for op, ln in ops:
        if op == 0:
            for _ in range(ln):
                if left > 0:
                    out.append(letter(Rv[i]))
                    left -= 1
                else:
                    t += 1
                    assert isinstance(toks[t], str) and toks[t][0] != "^", (md_string, t)
                    out.append(toks[t])
                    next_number()
                i += 1
        elif op == 1:
            i += ln
        else:
            assert left == 0, (md_string, t)
            t += 1
            assert toks[t][0] == "^" and len(toks[t]) == ln + 1, (md_string, t)
            out.append(toks[t][1:])
            next_number()
    assert left == 0 and t == len(toks) - 1, md_string
    return "".join(out)
