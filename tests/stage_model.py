"""What the stage calls of the sharded suffix sort (include/kiss_hip.h, the stage block) have to deliver, restated in plain
numpy / Python: suffix types, LMS positions, the 13 window counters, the emitted (key, position) list of a window, the k-order
of a list of far LMS suffixes, the tie groups and the layout of a context word.  No GPU, no library; held against the CPU
oracle by tests/test_stage_model.py and used as the reference by tests/test_stage_*_gpu.py.

Bases are 0..3 (A C G T).  The sentinel behind the text is smaller than every base.  D = depth_of(n, k) is the number of bases
the k-order compares; an LMS suffix p is far when p + D <= n (every one when D = 0 = exact order)."""
import numpy as np

STRIDE = 125
TILE = 8192          # bases per classification tile (256 packed words)
WORD = 32            # bases per packed word
KEY_BASES = 20       # key bits 63..24
KEY_CTX_BASES = 11   # context word inside the key, bits 23..0
CTX_BASES = 15       # context word of the placement step
TAINT = 0x80000000
HIST_BITS = 14


def depth_of(n, k):
    return 0 if k >= n else STRIDE * (k // STRIDE + 1)


_memo = {}  # per text (by identity; the text is kept alive and must not be written to): what does not depend on k or a window


def _once(S, what, make):
    slot = _memo.setdefault(id(S), {"S": S})
    assert slot["S"] is S
    if what not in slot:
        slot[what] = make()
    return slot[what]


def types(S):
    """1 = S-type, 0 = L-type; S[n-1] is L (the sentinel behind it is smaller)"""
    return _once(S, "types", lambda: _types(S))


def _types(S):
    n = len(S)
    t = np.zeros(n, dtype=np.int8)
    s = S.tolist()
    for i in range(n - 2, -1, -1):
        if s[i] < s[i + 1]:
            t[i] = 1
        elif s[i] == s[i + 1]:
            t[i] = t[i + 1]
    return t


def lms(S):
    """ascending LMS positions (S-type behind an L-type), the sentinel excluded"""
    t = types(S)
    return _once(S, "lms", lambda: np.array([i for i in range(1, len(S)) if t[i] == 1 and t[i - 1] == 0], dtype=np.int64))


def is_far(n, k, p):
    D = depth_of(n, k)
    return D == 0 or p + D <= n


def counts13(S, k, lo, hi):
    """count[c], s_count[c], lms_count[c] (c = A C G T) and the number of far LMS positions, all of the window [lo, hi)"""
    n = len(S)
    t = types(S)

    def first12():
        count, s_count, lms_count, where = [0] * 4, [0] * 4, [0] * 4, []
        for i in range(lo, hi):
            c = int(S[i])
            count[c] += 1
            if t[i] == 1:
                s_count[c] += 1
                if i > 0 and t[i - 1] == 0:
                    lms_count[c] += 1
                    where.append(i)
        return count + s_count + lms_count, where
    twelve, where = _once(S, ("counts", lo, hi), first12)  # (k enters the far count alone)
    return twelve + [sum(1 for i in where if is_far(n, k, i))]


def ctx_word(S, p, bases):
    """context word of position p: marker bit above j = min(p, bases) two-bit fields, base p - i in bits 2i-1 : 2i-2"""
    j = min(p, bases)
    w = 1 << (2 * j)
    for i in range(1, j + 1):
        w |= int(S[p - i]) << (2 * i - 2)
    return w


def key_of(S, p):
    """the emitted 64-bit key of position p: 20 bases from p on (A behind the end), then the 11-base context word"""
    n = len(S)
    key = 0
    for i in range(KEY_BASES):
        key = (key << 2) | (int(S[p + i]) if p + i < n else 0)
    return (key << 24) | ctx_word(S, p, KEY_CTX_BASES)


def local_list(S, k, lo, hi):
    """-> (keys u64, pos u32, m_far_local): the LMS positions of [lo, hi) ascending; the far ones are a prefix"""
    n = len(S)
    L = lms(S)
    pos = [int(p) for p in L[np.searchsorted(L, lo):np.searchsorted(L, hi)]]  # lo <= p < hi
    m_far = sum(1 for p in pos if is_far(n, k, p))
    assert all(is_far(n, k, p) for p in pos[:m_far])
    all_keys = _once(S, "keys", lambda: {int(p): key_of(S, int(p)) for p in lms(S)})  # (a key depends on p alone)
    return (np.array([all_keys[p] for p in pos], dtype=np.uint64), np.array(pos, dtype=np.uint32), m_far)


def key_hist(keys, bits=HIST_BITS):
    return np.bincount((np.asarray(keys, dtype=np.uint64) >> np.uint64(64 - bits)).astype(np.int64), minlength=1 << bits)


def valid_ctx_word(S, p, w):
    """a word coming back from the sort: taint aside, 0 ("gather it") or the context word of p with 11 or 15 bases"""
    w = int(w) & ~TAINT & 0xFFFFFFFF
    return w == 0 or w == ctx_word(S, int(p), KEY_CTX_BASES) or w == ctx_word(S, int(p), CTX_BASES)


def suffix_ranks(S):
    """rank of every suffix in the exact order (sentinel smallest), by prefix doubling"""
    return _once(S, "ranks", lambda: _suffix_ranks(S))


def _suffix_ranks(S):
    n = len(S)
    rank = np.asarray(S, dtype=np.int64) + 1
    h = 1
    while True:
        second = np.zeros(n, dtype=np.int64)  # 0 = the sentinel and what is behind it
        if h < n:
            second[:n - h] = rank[h:]
        order = np.lexsort((second, rank))
        differs = (rank[order][1:] != rank[order][:-1]) | (second[order][1:] != second[order][:-1])
        new = np.empty(n, dtype=np.int64)
        new[order] = np.concatenate([[1], 1 + np.cumsum(differs)])
        rank = new
        if int(rank.max()) == n or h >= n:
            return rank
        h *= 2


def suffix_array(S):
    """plain sort of all suffixes, the sentinel's (n) first"""
    return np.concatenate([[len(S)], np.argsort(suffix_ranks(S), kind="stable")]).astype(np.uint32)


def prefix(S, k, p):
    D = depth_of(len(S), k)
    return bytes(S[p:p + D])


def sort_list(S, k, pos):
    """k-order of an ascending list of far positions: stable sort by the D-base prefix; D = 0: by the whole suffix"""
    pos = [int(p) for p in pos]
    assert all(a < b for a, b in zip(pos, pos[1:])), "the list ascends by position"
    n = len(S)
    if depth_of(n, k) == 0:
        rank = suffix_ranks(S) if pos else None
        out = sorted(pos, key=lambda p: rank[p])
    else:
        assert all(is_far(n, k, p) for p in pos)
        out = sorted(pos, key=lambda p: prefix(S, k, p))  # (sorted is stable)
    return np.array(out, dtype=np.uint32)


def tied(S, k, pos):
    """the members of the list whose D-base prefix equals another member's (D > 0)"""
    assert depth_of(len(S), k) > 0
    groups = {}
    for p in pos:
        groups.setdefault(prefix(S, k, int(p)), []).append(int(p))
    return {p for g in groups.values() if len(g) > 1 for p in g}


def lcp_array(S):
    """lcp[r] = length of the common prefix of the suffixes of rank r - 1 and r in the exact order (Kasai's walk)"""
    def walk():
        n = len(S)
        sa = suffix_array(S)[1:].tolist()
        rank = (suffix_ranks(S) - 1).tolist()
        s = S.tolist()
        lcp, h = np.zeros(n, dtype=np.int64), 0
        for i in range(n):
            if rank[i] == 0:
                h = 0
                continue
            j = sa[rank[i] - 1]
            while i + h < n and j + h < n and s[i + h] == s[j + h]:
                h += 1
            lcp[rank[i]] = h
            h = max(h - 1, 0)
        return lcp
    return _once(S, "lcp", walk)


def max_common_prefix(S, pos):
    """the longest common prefix of two members of the list: what an exact-order sort of it has to compare through"""
    if len(pos) < 2:
        return 0
    lcp = lcp_array(S)
    r = np.sort(suffix_ranks(S)[np.asarray(pos, dtype=np.int64)] - 1)
    return max(int(lcp[a + 1:b + 1].min()) for a, b in zip(r[:-1].tolist(), r[1:].tolist()))
