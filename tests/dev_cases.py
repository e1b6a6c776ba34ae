"""One small case per device entry point that takes a stream, for tests/test_dev_placement_gpu.py (where the caller's
arrays lie) and tests/test_dev_stream_gpu.py (which stream the work runs on).  No GPU code here: a case knows its input
arrays, a DECOY -- another valid input of the same shapes whose every output differs --, what the model or the oracle says
the outputs are, and how to call the C entry on a dict of device addresses.  tests/test_dev_place_model.py holds the list
against include/kiss_hip.h.

A case's data(which), which = "real" or "decoy", gives
  inp   name -> numpy array: the device inputs (the arrays of an index view too)
  outs  name -> numpy array: every device output, exactly as many elements as the entry is given room for
  scal  name -> value: the return code, returned totals and the report fields the model defines
  host  whatever call() needs beside the addresses (sizes, parameters, the scalar fields of a view)
and call(lib, ctx, p, host, stream) runs the entry on the addresses p[name] and returns its scal.
"""
import ctypes
import functools

import numpy as np

from kiss_amd import _lib
from tests import dev_place, gen
from tests import fm8_model, fm_align_model, fm_chain_model, fm_mm_model, fm_model, fm_pair_model, fm_rescue_model
from tests import fm_seed_model, fm_select_model, lcp_model, verify_model

U8, U16, U32, U64 = np.uint8, np.uint16, np.uint32, np.uint64
K_UNBOUNDED = 0xFFFFFFFF
VP = ctypes.c_void_p


def lead_of(array, second=False):
    """the offset a caller may give an array of this element type (dev_place.LEADS); a byte array has two, 1 and 3"""
    size = np.asarray(array).dtype.itemsize
    if size == 1:
        return dev_place.LEADS["u8"][1 if second else 0]
    return {2: 2, 4: 4, 8: 8}[size]


class Data:
    def __init__(self, inp, outs, scal, host=None):
        self.inp = {k: np.ascontiguousarray(v) for k, v in inp.items()}
        self.outs = {k: np.ascontiguousarray(v) for k, v in outs.items()}
        self.scal, self.host = scal, host or {}


class Case:
    entry = None
    max_n = 1 << 20
    in_stream_test = True   # False: a case the placement file alone runs (its decoy could not differ: n = 1, ...)
    leads = {}              # name -> lead, where the element type does not say it (a 16-byte aligned bwt)
    constant = ()           # arrays that hold the same for every input of these shapes: no decoy can differ there

    def __init__(self, name, **kw):
        self.name = name
        self.kw = kw
        self._data = {}

    @property
    def id(self):
        return "%s-%s" % (self.entry.replace("kiss_hip_", ""), self.name)

    def data(self, which):
        if which not in self._data:
            self._data[which] = self.make({"real": 0, "decoy": 1}[which])
        return self._data[which]

    def byte_names(self):
        """the byte arrays of the case, inputs and outputs, in the order of their names"""
        d = self.data("real")
        return sorted(k for k, v in list(d.inp.items()) + list(d.outs.items()) if v.dtype.itemsize == 1 and k not in self.leads)

    def lead(self, name, array, flip=0):
        """Where `name` is placed.  Byte arrays take turns between 1 and 3 in the order of their names, so that neighbours
        differ, and `flip` = 1 exchanges the two: over flip = 0 and 1 EVERY byte array lies at 1 and at 3."""
        if name in self.leads:
            return self.leads[name]
        if np.asarray(array).dtype.itemsize == 1:
            return lead_of(array, second=(self.byte_names().index(name) + flip) % 2 == 1)
        return lead_of(array)

    def make(self, variant):
        raise NotImplementedError

    def call(self, lib, ctx, p, host, stream):
        raise NotImplementedError

    def defined(self, name, host):
        """the part of output `name` whose content the header defines (all of it, but for parse_text's spare room)"""
        return slice(None)

    def normalise(self, outs, host):
        """outputs as they are compared (fmi8 query: a pattern without a hit has no defined beg)"""
        return outs


def oracle():
    from tests import oracle_binding
    return oracle_binding.load()


def csr(counts, first=0):
    return np.concatenate([[first], first + np.cumsum(np.asarray(counts, np.int64))]).astype(U64)


def rows_u32(rows, width):
    return np.asarray(rows, np.int64).reshape(-1, width).astype(U32)


def report_of(rep, keys):
    out = {}
    for k in keys:
        v = getattr(rep, k)
        out[k] = [int(x) for x in v] if hasattr(v, "__len__") else int(v)
    return out


@functools.lru_cache(maxsize=None)
def dna_text(n, seed):
    """n bases; from 2 000 up with a stretch that occurs twice (REPEAT_AT says where), from 4 099 up with a run of one base as
    well, so that ties reach past one key"""
    S = gen.iid(n, 1000 + seed)
    if n >= 2000:
        src, dst, ln = repeat_at(n)
        S[dst:dst + ln] = S[src:src + ln]
    if n >= 4099:
        S[n // 2:n // 2 + 100] = seed & 3
    return S


def repeat_at(n):
    return n // 40, 3 * n // 4, n // 10


@functools.lru_cache(maxsize=None)
def exact_sa(n, seed):
    return oracle().suffix_sort(dna_text(n, seed), K_UNBOUNDED)


# ---- suffix sorting ---------------------------------------------------------------------------------------------------------
class SortDna(Case):
    entry = "kiss_hip_ctx_suffix_sort_dna_u32_dev"

    def make(self, variant):
        n, k, algo = self.kw["n"], self.kw["k"], self.kw["algo"]
        S = dna_text(n, 10 + variant)
        SA = oracle().suffix_sort(S, k)
        return Data(dict(S=S), dict(SA=SA.astype(U32)), dict(rc=0), dict(n=n, k=k, algo=algo))

    def call(self, lib, ctx, p, host, stream):
        rc = lib.kiss_hip_ctx_suffix_sort_dna_u32_dev(ctx, VP(p["S"]), host["n"], host["k"], host["algo"], VP(p["SA"]), VP(stream))
        return dict(rc=rc)


def byte_text(kind, n, variant):
    if kind == "english":
        return fm8_model.english_like(n, 5 + variant)
    return fm8_model.families(n, 7 + variant)[kind]


class SortU8(Case):
    entry = "kiss_hip_ctx_suffix_sort_u8_dev"

    def make(self, variant):
        S = byte_text(self.kw["kind"], self.kw["n"], variant)
        SA = fm8_model.exact_sa_doubling(S)
        return Data(dict(S=np.frombuffer(S, U8)), dict(SA=SA), dict(rc=0), dict(n=len(S)))

    def call(self, lib, ctx, p, host, stream):
        return dict(rc=lib.kiss_hip_ctx_suffix_sort_u8_dev(ctx, VP(p["S"]), host["n"], VP(p["SA"]), VP(stream)))


class VerifySa(Case):
    entry = "kiss_hip_ctx_verify_sa_dev"
    # no output array: the report is what a decoy has to change -- the digest (the kernel that reads SA alone) AND what the
    # order kernels count (they read S and SA), so that neither can run on the decoy unnoticed
    must_differ = ("digest", "first_violation", "order_violations")

    def make(self, variant):
        n, k = self.kw["n"], self.kw["k"]
        S = dna_text(n, 20 + variant)
        SA = oracle().suffix_sort(S, k).copy()
        if self.kw.get("damage"):  # two entries exchanged: violations to count, and still a permutation
            i, j = 17 + variant, n // 2 + 3 * variant
            SA[i], SA[j] = SA[j], SA[i]
            if variant and n > 100:  # (another number of violations than the real input's)
                SA[n - 9], SA[n // 3] = SA[n // 3], SA[n - 9]
        want = verify_model.report(S, SA, k)
        scal = dict(rc=0, n=n, k=k)
        scal.update({f: want[f] for f in verify_model.comparable(want)})
        return Data(dict(S=S, SA=SA.astype(U32)), {}, scal, dict(n=n, k=k))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.VerifyReport()
        rc = lib.kiss_hip_ctx_verify_sa_dev(ctx, VP(p["S"]), host["n"], host["k"], VP(p["SA"]), ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("n", "k") + verify_model.FIELDS)
        scal["rc"] = rc
        return scal


class Lcp(Case):
    def make(self, variant):
        n = self.kw["n"]
        if self.entry.endswith("_u8_dev"):
            raw = byte_text("english", n, variant)
            S, SA = np.frombuffer(raw, U8), fm8_model.exact_sa_doubling(raw)
        else:
            S = dna_text(n, 30 + variant)
            SA = oracle().suffix_sort(S, K_UNBOUNDED)
        LCP = lcp_model.kasai(S, SA)
        scal = dict(rc=0, n=n, lcp_sum=int(LCP.astype(np.uint64).sum()), max_lcp=int(LCP.max()))
        return Data(dict(S=S, SA=SA.astype(U32)), dict(LCP=LCP), scal, dict(n=n))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.LcpReport()
        rc = getattr(lib, self.entry)(ctx, VP(p["S"]), host["n"], VP(p["SA"]), VP(p["LCP"]), ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("n", "lcp_sum", "max_lcp"))
        scal["rc"] = rc
        return scal


class LcpDna(Lcp):
    entry = "kiss_hip_ctx_lcp_dna_u32_dev"


class LcpU8(Lcp):
    entry = "kiss_hip_ctx_lcp_u8_dev"


def fasta_bytes(total, variant, plain=False):
    """a file of exactly `total` bytes: records with headers, lower case, N, CR LF, an empty line, '>' inside a line"""
    rng = np.random.default_rng(40 + variant)
    out = bytearray()
    rec = 0
    while len(out) < total:
        if not plain:
            out += b">rec%d some words %d\n" % (rec, int(rng.integers(0, 10 ** (1 + variant))))
        for _ in range(int(rng.integers(1, 9))):
            width = int(rng.integers(1, 90))
            line = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTacgtNnRY", U8), width))
            out += line + (b"\r\n" if rng.random() < 0.1 else b"\n")
        if rng.random() < 0.3:
            out += b"\n"
        rec += 1
    return bytes(out[:total - 1]) + b"\n"


class ParseText(Case):
    entry = "kiss_hip_ctx_parse_text_dev"

    def make(self, variant):
        raw = fasta_bytes(self.kw["bytes"], variant, self.kw.get("plain", False))
        codes = oracle().read_sequence(raw)
        host = dict(bytes=len(raw), n=int(codes.size))
        # the header asks for room for `bytes` codes; the n codes are compared, the rest of the room is not defined
        S = np.full(len(raw), 0xEE, U8)
        S[:codes.size] = codes
        return Data(dict(raw=np.frombuffer(raw, U8)), dict(S=S), dict(rc=0, n=int(codes.size)), host)

    def call(self, lib, ctx, p, host, stream):
        n = ctypes.c_uint64()
        rc = lib.kiss_hip_ctx_parse_text_dev(ctx, VP(p["raw"]), host["bytes"], VP(p["S"]), ctypes.byref(n), VP(stream))
        return dict(rc=rc, n=int(n.value))

    def defined(self, name, host):
        return slice(0, host["n"])


# ---- the DNA index ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fm_of(n, seed, sa_intv, lookup_len):
    return fm_model.FmModel(dna_text(n, seed), exact_sa(n, seed), sa_intv, lookup_len)


def fm_arrays(m):
    """the arrays of a kiss_hip_fmi_view(_ex) from tests/fm_model.py, packed as the .fmi file has them"""
    N = m.N
    d = np.concatenate([m.bwt, np.zeros((-N) % 4, U8)]).reshape(-1, 4).astype(U8)
    out = dict(bwt=(d[:, 0] | (d[:, 1] << 2) | (d[:, 2] << 4) | (d[:, 3] << 6)).astype(U8), occ1=m.occ1.astype(U32).reshape(-1),
               occ2=m.occ2.astype(U8).reshape(-1), sa=m.sa.astype(U32))
    if m.sa_intv != 1:
        bits = np.concatenate([m.b, np.zeros((-N) % 64, bool)])
        out["b"] = np.packbits(bits, bitorder="little").view(U64)
        out["b_occ"] = m.b_occ.astype(U32)
    return out


def fm_view(m, p, ex=False, with_lookup=True):
    v = _lib.FmiView()
    v.n_sa = m.N
    for c in range(4):
        v.cnt[c] = int(m.cnt[c])
    v.pri, v.sa_intv = m.pri, m.sa_intv
    v.bwt, v.occ1, v.occ2, v.sa = p["bwt"], p["occ1"], p["occ2"], p["sa"]
    if m.sa_intv != 1:
        v.b, v.b_occ = p["b"], p["b_occ"]
    if not ex:
        return v
    vex = _lib.FmiViewEx()
    vex.base = v
    vex.lookup_len = m.lookup_len if with_lookup else 0
    vex.lookup = p["lookup"] if with_lookup else None
    return vex


def patterns_of(S, Q, L, seed):
    rng = np.random.default_rng(seed)
    pats = rng.integers(0, 4, (Q, L), dtype=U8)
    for q in range(Q):
        if q % 3:  # (every third one stays random; the others occur)
            at = int(rng.integers(0, S.size - L + 1))
            pats[q] = S[at:at + L]
    pats[Q - 1] = S[S.size - L:]  # the pattern that ends the text
    return pats


class FmBuild(Case):
    entry = "kiss_hip_fmi_build_dev"

    def make(self, variant):
        n = self.kw["n"]
        sa_intv, lookup_len = self.kw.get("sa_intv", 4), self.kw.get("lookup_len", 0)
        m = fm_of(n, 50 + variant, sa_intv, lookup_len)
        outs = fm_arrays(m)
        if self.entry.endswith("_ex_dev"):
            outs["lookup"] = m.lookup.astype(U32)
        scal = dict(rc=0, cnt=[int(x) for x in m.cnt], pri=m.pri)
        return Data(dict(S=dna_text(n, 50 + variant), SA=exact_sa(n, 50 + variant).astype(U32)), outs, scal,
                    dict(n=n, sa_intv=sa_intv, lookup_len=lookup_len))

    def call(self, lib, ctx, p, host, stream):
        cnt, pri = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
        rc = lib.kiss_hip_fmi_build_dev(ctx, VP(p["S"]), host["n"], VP(p["SA"]), host["sa_intv"], VP(p["bwt"]), VP(p["occ1"]),
                                        VP(p["occ2"]), VP(p["sa"]), VP(p["b"]), VP(p["b_occ"]), ctypes.byref(cnt), ctypes.byref(pri),
                                        VP(stream))
        return dict(rc=rc, cnt=[int(x) for x in cnt], pri=int(pri.value))


class FmBuildEx(FmBuild):
    entry = "kiss_hip_fmi_build_ex_dev"

    def call(self, lib, ctx, p, host, stream):
        cnt, pri = (ctypes.c_uint32 * 4)(), ctypes.c_uint32()
        rc = lib.kiss_hip_fmi_build_ex_dev(ctx, VP(p["S"]), host["n"], VP(p["SA"]), host["sa_intv"], host["lookup_len"], VP(p["bwt"]),
                                           VP(p["occ1"]), VP(p["occ2"]), VP(p["sa"]), VP(p.get("b")), VP(p.get("b_occ")),
                                           VP(p["lookup"]), ctypes.byref(cnt), ctypes.byref(pri), VP(stream))
        return dict(rc=rc, cnt=[int(x) for x in cnt], pri=int(pri.value))


class FmQuery(Case):
    entry = "kiss_hip_fmi_query_batch_dev"
    ex = False

    def make(self, variant):
        n, Q, L = self.kw["n"], self.kw.get("Q", 9), self.kw.get("L", 20)
        sa_intv, lookup_len, stop_cnt = self.kw.get("sa_intv", 4), self.kw.get("lookup_len", 0), self.kw.get("stop_cnt", 0)
        m = fm_of(n, 60 + variant, sa_intv, lookup_len)
        pats = patterns_of(dna_text(n, 60 + variant), Q, L, 61 + variant)
        want = m.query_batch(pats, stop_cnt)
        inp = fm_arrays(m)
        inp["patterns"] = pats.reshape(-1)
        outs = dict(beg=want["beg"], end=want["end"], offsets=want["offsets"], offsets_index=want["offsets_index"])
        if self.ex:
            inp["lookup"] = m.lookup.astype(U32)
            outs["offs"] = want["offs"]
        assert want["total_hits"] > 0
        scal = dict(rc=0, total=want["total_hits"], checksum=want["checksum"])
        return Data(inp, outs, scal, dict(m=m, Q=Q, L=L, stop_cnt=stop_cnt, cap=int(want["offsets"].size)))

    def call(self, lib, ctx, p, host, stream):
        tot, chk = ctypes.c_uint64(), ctypes.c_uint64()
        if self.ex:
            view = fm_view(host["m"], p, ex=True)
            rc = lib.kiss_hip_fmi_query_ex_dev(ctx, ctypes.byref(view), VP(p["patterns"]), host["L"], host["Q"], host["stop_cnt"],
                                               VP(p["beg"]), VP(p["end"]), VP(p["offs"]), ctypes.byref(tot), ctypes.byref(chk),
                                               VP(p["offsets"]), VP(p["offsets_index"]), host["cap"], VP(stream))
        else:
            view = fm_view(host["m"], p)
            rc = lib.kiss_hip_fmi_query_batch_dev(ctx, ctypes.byref(view), VP(p["patterns"]), host["L"], host["Q"], VP(p["beg"]),
                                                  VP(p["end"]), ctypes.byref(tot), ctypes.byref(chk), VP(p["offsets"]),
                                                  VP(p["offsets_index"]), host["cap"], VP(stream))
        return dict(rc=rc, total=int(tot.value), checksum=int(chk.value))


class FmQueryEx(FmQuery):
    entry = "kiss_hip_fmi_query_ex_dev"
    ex = True


class FmQueryMm(Case):
    entry = "kiss_hip_fmi_query_mm_dev"

    def make(self, variant):
        n, Q, L, e = self.kw["n"], 9, 20, 2
        S = dna_text(n, 70 + variant)
        m = fm_of(n, 70 + variant, 4, 0)
        pats = patterns_of(S, Q, L, 71 + variant)
        for q in range(1, Q, 2):  # one base changed: hits with one mismatch
            pats[q, 3 + q] = (pats[q, 3 + q] + 1) & 3
        counts, pos, mis, idx = fm_mm_model.brute_batch(S, pats, e)
        inp = fm_arrays(m)
        inp["patterns"] = pats.reshape(-1)
        outs = dict(counts=counts.astype(U32).reshape(-1), positions=pos.astype(U32), mismatches=mis.astype(U8), index=idx.astype(U64))
        hits = counts.sum(axis=0).tolist() + [0] * (3 - e)
        assert pos.size > 0 and hits[0] > 0 and hits[1] > 0
        scal = dict(rc=0, Q=Q, L=L, max_mismatches=e, hits=[int(x) for x in hits], walk_failures=0, checksum=int(pos.sum()))
        return Data(inp, outs, scal, dict(m=m, Q=Q, L=L, e=e, cap=int(pos.size)))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.FmiMmReport()
        view = fm_view(host["m"], p)
        rc = lib.kiss_hip_fmi_query_mm_dev(ctx, ctypes.byref(view), VP(p["patterns"]), host["L"], host["Q"], host["e"], VP(p["counts"]),
                                           VP(p["positions"]), VP(p["mismatches"]), VP(p["index"]), host["cap"], ctypes.byref(rep),
                                           VP(stream))
        scal = report_of(rep, ("Q", "L", "max_mismatches", "hits", "walk_failures", "checksum"))
        scal["rc"] = rc
        return scal


# ---- the byte index -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fm8_of(n, variant, sa_intv):
    raw = byte_text("english", n, variant)
    if variant:  # other byte values, as many of them: the arrays keep their sizes
        raw = bytes(np.frombuffer(raw, U8) ^ 0x80)
    return fm8_model.Model(raw, sa_intv, SA=fm8_model.exact_sa_doubling(raw))


def fm8_arrays(m):
    """the arrays of a kiss_hip_fmi8_view from tests/fm8_model.py (include/kiss_hip.h says what they hold)"""
    N, sigma = m.N, m.sigma
    nblk, nsb = N // 256 + 1, N // 65536 + 1
    bwt = np.zeros(nblk * 256, U8)
    bwt[:N] = m.bwt
    codes = m.map[m.bwt].astype(np.int64)
    codes[m.pri] = -1
    occ1, occ2 = np.zeros((sigma, nsb), U32), np.zeros((sigma, nblk), U16)
    for c in range(sigma):
        before = np.concatenate(([0], np.cumsum(codes == c)))
        at_blk = before[np.minimum(np.arange(nblk) * 256, N)]
        at_sb = before[np.minimum(np.arange(nsb) * 65536, N)]
        occ1[c] = at_sb
        occ2[c] = at_blk - at_sb[np.arange(nblk) // 256]
    out = dict(C=m.C.astype(U32), map=m.map.astype(U8), bwt=bwt, occ1=occ1.reshape(-1), occ2=occ2.reshape(-1), sa=m.sa.astype(U32))
    if m.sa_intv != 1:
        bits = np.concatenate([m.sampled, np.zeros((-N) % 64, bool)])
        out["b"] = np.packbits(bits, bitorder="little").view(U64)
        out["b_occ"] = np.concatenate(([0], np.cumsum(m.sampled)))[np.arange(N // 64 + 1) * 64].astype(U32)
    return out


class Fm8Build(Case):
    entry = "kiss_hip_fmi8_build_dev"
    leads = {"bwt": 16}  # the header demands 16 bytes of bwt: tests/test_dev_placement_gpu.py tests the refusal of less
    constant = ("occ1",)  # below 65 536 rows there is one superblock, and occ1 holds the counts in front of it: zeros

    def make(self, variant):
        n, sa_intv = self.kw["n"], self.kw.get("sa_intv", 4)
        m = fm8_of(n, variant, sa_intv)
        scal = dict(rc=0, sigma=m.sigma, pri=m.pri)
        return Data(dict(S=np.frombuffer(m.S, U8), SA=m.SA.astype(U32)), fm8_arrays(m), scal, dict(n=n, sa_intv=sa_intv, sigma=m.sigma))

    def call(self, lib, ctx, p, host, stream):
        sigma, pri = ctypes.c_uint32(), ctypes.c_uint32()
        rc = lib.kiss_hip_fmi8_build_dev(ctx, VP(p["S"]), host["n"], VP(p["SA"]), host["sa_intv"], host["sigma"], VP(p["C"]), VP(p["map"]),
                                         VP(p["bwt"]), VP(p["occ1"]), VP(p["occ2"]), VP(p["sa"]), VP(p.get("b")), VP(p.get("b_occ")),
                                         ctypes.byref(sigma), ctypes.byref(pri), VP(stream))
        return dict(rc=rc, sigma=int(sigma.value), pri=int(pri.value))


class Fm8Query(Case):
    entry = "kiss_hip_fmi8_query_dev"
    leads = {"bwt": 16}
    constant = ("occ1",)

    def make(self, variant):
        n, sa_intv = self.kw["n"], self.kw.get("sa_intv", 4)
        m = fm8_of(n, variant, sa_intv)
        pats = fm8_model.patterns_for(m.S, 9, 80, max_len=300)  # (the lengths depend on the seed alone)
        if variant:
            pats = pats[::-1]
        counts, index, positions, checksum = fm8_model.brute_batch(m.S, pats)
        ranges = [m.search(P) for P in pats]
        inp = fm8_arrays(m)
        inp["patterns"] = np.frombuffer(b"".join(pats), U8)
        inp["pat_index"] = csr([len(P) for P in pats])
        outs = dict(beg=np.array([r[0] for r in ranges], U32), end=np.array([r[1] for r in ranges], U32), positions=positions,
                    index=index.astype(U64))
        assert positions.size > len(pats)
        scal = dict(rc=0, total=int(counts.sum()), checksum=checksum, Q=len(pats), hits=int(counts.sum()), walk_failures=0,
                    rep_checksum=checksum)
        return Data(inp, outs, scal, dict(m=m, Q=len(pats), cap=int(positions.size), counts=counts))

    def view(self, m, p):
        v = _lib.Fmi8View()
        v.n_sa, v.pri, v.sa_intv, v.sigma = m.N, m.pri, m.sa_intv, m.sigma
        for k in ("C", "map", "bwt", "occ1", "occ2", "sa"):
            setattr(v, k, p[k])
        if m.sa_intv != 1:
            v.b, v.b_occ = p["b"], p["b_occ"]
        return v

    def call(self, lib, ctx, p, host, stream):
        tot, chk, rep = ctypes.c_uint64(), ctypes.c_uint64(), _lib.Fmi8Report()
        v = self.view(host["m"], p)
        rc = lib.kiss_hip_fmi8_query_dev(ctx, ctypes.byref(v), VP(p["patterns"]), VP(p["pat_index"]), host["Q"], VP(p["beg"]),
                                         VP(p["end"]), ctypes.byref(tot), ctypes.byref(chk), VP(p["positions"]), VP(p["index"]),
                                         host["cap"], ctypes.byref(rep), VP(stream))
        return dict(rc=rc, total=int(tot.value), checksum=int(chk.value), Q=int(rep.Q), hits=int(rep.hits),
                    walk_failures=int(rep.walk_failures), rep_checksum=int(rep.checksum))

    def normalise(self, outs, host):
        """a pattern without a hit has beg == end and no defined value of either (include/kiss_hip.h): compare them as 0, 0"""
        beg, end = outs["beg"].copy(), outs["end"].copy()
        none = beg == end
        beg[none] = end[none] = 0
        return dict(outs, beg=beg, end=end)


# ---- reads: seeds, chains, alignments ----------------------------------------------------------------------------------------------
def revcomp(R):
    return fm_seed_model.revcomp(R)


def mutate(piece, rng, subs=2, indels=2):
    """a piece of text with substitutions and 1..3-base insertions and deletions"""
    R = np.asarray(piece, U8).copy()
    for _ in range(subs):
        j = int(rng.integers(0, R.size))
        R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
    for _ in range(indels):
        j, g = int(rng.integers(4, R.size - 4)), int(rng.integers(1, 4))
        R = np.concatenate([R[:j], rng.integers(0, 4, g, dtype=U8), R[j:]]) if rng.random() < 0.5 else np.concatenate([R[:j], R[j + g:]])
    return R


READ_LENGTHS = (100, 300, 150, 101, 257, 120)


def reads_of(S, lengths, seed):
    """per length a read cut from the text with about 2 % substitutions, every second one reverse-complemented, one with a
    no-base in the middle, one that ends the text"""
    rng = np.random.default_rng(seed)
    out = []
    for q, L in enumerate(lengths):
        at = S.size - L if q == 3 else int(rng.integers(0, S.size - L + 1))
        if q == 0:  # inside the stretch that occurs twice: seeds with two positions
            at = repeat_at(S.size)[0] + 10
        R = S[at:at + L].copy()
        for j in rng.choice(L, max(1, L // 50), replace=False):
            R[j] = (R[j] + 1 + rng.integers(0, 3)) & 3
        if q == 2:
            R[L // 2] = 78  # 'N'
        out.append(revcomp(R) if q % 2 else R)
    return out


class Seeds(Case):
    entry = "kiss_hip_fmi_seeds_dev"

    def make(self, variant):
        n, both = self.kw["n"], self.kw["both"]
        min_len, max_len, max_occ = 19, 0, 500
        S = dna_text(n, 90 + variant)
        m = fm_of(n, 90 + variant, 4, 0)
        lengths = READ_LENGTHS if not variant else READ_LENGTHS[::-1]
        reads = reads_of(S, lengths, 91 + variant)
        b = fm_seed_model.Batch(S, reads, both, max_len)
        want = b.seeds(min_len, max_occ)
        # the range of every seed string: get_range of the model index, one call per length
        nseeds = want["len"].size
        rec = np.zeros((nseeds, 4), U32)
        rec[:, 0], rec[:, 1] = want["start"], want["len"]
        for L in np.unique(want["len"]).tolist():
            rows = np.flatnonzero(want["len"] == L)
            pats = np.stack([np.frombuffer(want["strings"][i], U8) for i in rows])
            beg, end, _ = m.get_ranges(pats)
            rec[rows, 2], rec[rows, 3] = beg, end
        assert np.array_equal(rec[:, 3].astype(np.int64) - rec[:, 2], want["count"])
        inp = fm_arrays(m)
        inp["reads"] = np.concatenate(reads)
        inp["read_index"] = csr([r.size for r in reads])
        outs = dict(ms=b.ms.astype(U32), seeds=rec.reshape(-1), seed_index=want["seed_index"].astype(U64),
                    positions=want["positions"].astype(U32), pos_index=want["pos_index"].astype(U64))
        assert nseeds >= len(reads) and want["positions"].size >= nseeds
        scal = dict(rc=0, Q=b.Q, V=b.V, bases=b.bases, seeds=nseeds, located_seeds=want["located_seeds"],
                    positions=int(want["positions"].size), lf_pairs=b.lf_pairs, walk_failures=0, checksum=want["checksum"],
                    max_ms=int(b.ms.max()))
        host = dict(m=m, Q=len(reads), both=1 if both else 0, params=(min_len, max_len, max_occ), seed_cap=nseeds,
                    pos_cap=int(want["positions"].size))
        return Data(inp, outs, scal, host)

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.FmiSeedReport()
        vex = fm_view(host["m"], p, ex=True, with_lookup=False)
        rc = lib.kiss_hip_fmi_seeds_dev(ctx, ctypes.byref(vex), VP(p["reads"]), VP(p["read_index"]), host["Q"], *host["params"],
                                        host["both"], VP(p["ms"]), VP(p["seeds"]), VP(p["seed_index"]), host["seed_cap"],
                                        VP(p["positions"]), VP(p["pos_index"]), host["pos_cap"], ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("Q", "V", "bases", "seeds", "located_seeds", "positions", "lf_pairs", "walk_failures", "checksum",
                               "max_ms"))
        scal["rc"] = rc
        return scal


def chain_read(rng, nseeds, pos_counts):
    """seeds with one to three positions each near two diagonals, many equal coordinates (tests/test_fm_chain_gpu.py)"""
    out = []
    for i in range(nseeds):
        r = int(rng.integers(0, 200))
        ps = sorted(int(r + 1000 * rng.integers(0, 2) + 4 * rng.integers(-3, 4)) + 100 for _ in range(pos_counts[i]))
        out.append((r, int(rng.integers(1, 40)), ps))
    return out


class Chain(Case):
    entry = "kiss_hip_fmi_chain_dev"
    PARAMS = dict(max_gap=300, band=30, min_score=20)

    def make(self, variant):
        rng = np.random.default_rng(100 + variant)
        seed_counts = [40, 0, 25, 40, 33]
        pos_counts = [1 + (i * 7) % 3 for i in range(sum(seed_counts))]
        if variant:  # the same totals, every index another
            seed_counts, pos_counts = seed_counts[::-1], pos_counts[::-1]
        start, length, pos, pidx, at = [], [], [], [0], 0
        for c in seed_counts:
            for s, l, ps in chain_read(rng, c, pos_counts[at:at + c]):
                start.append(s)
                length.append(l)
                pos += ps
                pidx.append(len(pos))
            at += c
        sidx = csr(seed_counts)
        want = fm_chain_model.chain(start, length, sidx, pos, pidx, **self.PARAMS)
        seeds = np.zeros((len(start), 4), U32)
        seeds[:, 0], seeds[:, 1] = start, length
        seeds[:, 2] = 5 + variant  # (sa_beg / sa_end: not read by the chain call)
        inp = dict(seeds=seeds.reshape(-1), seed_index=sidx, positions=np.asarray(pos, U32), pos_index=np.asarray(pidx, U64))
        outs = dict(chains=rows_u32(want["chains"], 6).reshape(-1), chain_index=want["chain_index"].astype(U64),
                    chain_anchors=rows_u32(want["anchors"], 3).reshape(-1), anchor_index=want["anchor_index"].astype(U64))
        nch, nanc = want["chains"].shape[0], want["anchors"].shape[0]
        assert nch > 2 and nanc > nch
        scal = dict(rc=0, V=want["V"], anchors=want["n_anchors"], chains=nch, chain_anchors=nanc, dp_pairs=want["dp_pairs"],
                    max_anchors=want["max_anchors"], best_score=want["best_score"])
        return Data(inp, outs, scal, dict(V=len(seed_counts), chain_cap=nch, anchor_cap=nanc))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.ChainReport()
        params = _lib.ChainParams(**fm_chain_model.params_of(**self.PARAMS))
        rc = lib.kiss_hip_fmi_chain_dev(ctx, VP(p["seeds"]), VP(p["seed_index"]), host["V"], VP(p["positions"]), VP(p["pos_index"]),
                                        ctypes.byref(params), VP(p["chains"]), VP(p["chain_index"]), host["chain_cap"],
                                        VP(p["chain_anchors"]), VP(p["anchor_index"]), host["anchor_cap"], ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("V", "anchors", "chains", "chain_anchors", "dp_pairs", "max_anchors", "best_score"))
        scal["rc"] = rc
        return scal


class Align(Case):
    entry = "kiss_hip_fmi_align_dev"
    PARAMS = dict(band=9)

    def make(self, variant):
        n = self.kw["n"]
        rng = np.random.default_rng(110 + variant)
        S = dna_text(n, 110 + variant)
        places = (0, 300, 600, n - 125) if not variant else (n - 125, 40, 900, 1300)
        reads, quads = [], []
        for q, at in enumerate(places):
            L = 120 + (3 - q if variant else q)
            R = mutate(S[at:at + L], rng)[:L]
            R = np.concatenate([R, rng.integers(0, 4, L - R.size, dtype=U8)])
            reads.append(revcomp(R) if q % 2 else R)
        # both strands: virtual read 2 q is read q, 2 q + 1 its reverse complement; the chains sit where the text matches
        counts = [1, 0, 0, 2, 1, 1, 0, 1] if not variant else [1, 1, 0, 1, 2, 0, 0, 1]
        for v, c in enumerate(counts):
            L, at = reads[v // 2].size, places[v // 2]
            for j in range(c):
                quads.append((0, L, max(0, at + 5 * j - 2), min(n, at + L + 5 * j)))
        cidx = csr(counts, first=3 * variant)  # (chain_index need not start at 0: records in front that are not the call's)
        want = fm_align_model.align(S, reads, [(1, 2, 3, 4)] * (3 * variant) + quads, cidx, True, **self.PARAMS)
        C, ops = len(quads), int(want["cigar"].size)
        assert ops > C and (want["alignments"][:, 0] > 50).sum() >= 4
        chains = np.zeros((3 + C, 6), U32)  # (three records that are not the call's: in front of them, or behind)
        chains[3 * variant:3 * variant + C, 2:6] = np.asarray(quads, np.int64)
        chains[:, 0] = 7 + variant
        inp = dict(text=S, reads=np.concatenate(reads), read_index=csr([r.size for r in reads]), chains=chains.reshape(-1),
                   chain_index=cidx)
        outs = dict(alns=rows_u32(want["alignments"], 12).reshape(-1), cigar=want["cigar"].astype(U32),
                    cigar_index=want["cigar_index"].astype(U64))
        scal = dict(rc=0, V=8, chains=C, aligned=want["aligned"], too_wide=want["too_wide"], cells=want["cells"], cigar_ops=ops,
                    best_score=want["best_score"], max_band=want["max_band"])
        return Data(inp, outs, scal, dict(n=n, Q=4, aln_cap=C, cigar_cap=ops))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.AlignReport()
        params = _lib.AlignParams(**fm_align_model.params_of(**self.PARAMS))
        rc = lib.kiss_hip_fmi_align_dev(ctx, VP(p["text"]), host["n"], VP(p["reads"]), VP(p["read_index"]), host["Q"], 1, VP(p["chains"]),
                                        VP(p["chain_index"]), ctypes.byref(params), VP(p["alns"]), host["aln_cap"], VP(p["cigar"]),
                                        VP(p["cigar_index"]), host["cigar_cap"], ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("V", "chains", "aligned", "too_wide", "cells", "cigar_ops", "best_score", "max_band"))
        scal["rc"] = rc
        return scal


# ---- records: select, pair, rescue, merge ------------------------------------------------------------------------------------------
def aln_rec(score, rbeg, rend, tbeg, tend, flags=0):
    return (score, flags, rbeg, rend, tbeg, tend, 0, 0, 0, 0, 0, 65)


def select_read(rng, count, L):
    """`count` records of one read, text starts drawn from a stretch of 8 bases per record: most are redundant to an earlier one"""
    out = []
    for _ in range(count):
        rb = int(rng.integers(0, L // 2))
        re = int(rng.integers(rb + L // 4, L + 1))
        tb = int(rng.integers(0, 8 * count + 200))
        out.append(aln_rec(int(rng.choice((40, 50, 60))), rb, re, tb, tb + (re - rb) + int(rng.integers(0, 3))))
    return out


class Select(Case):
    entry = "kiss_hip_fmi_select_dev"

    def make(self, variant):
        rng = np.random.default_rng(120 + variant)
        counts = [2, 1, 0, 0, 40, 30, 3, 2] if not variant else [3, 2, 30, 40, 0, 1, 0, 2]  # per virtual read, both strands
        lens = [150, 140, 160, 150] if not variant else [160, 150, 150, 140]
        rows = []
        for v, c in enumerate(counts):
            rows += select_read(rng, c, lens[v // 2])
        cidx = csr(counts, first=2 * variant)
        bounds = np.array([0, 330 + variant, 5000], U64)
        want = fm_select_model.select(rows, cidx, lens, both_strands=True, bounds=bounds)
        H = want["hits"].shape[0]
        assert H > 8 and want["report"]["spanning"] > 0 and want["report"]["redundant"] > 0 and len(set(want["hits"][:, 7])) == 2
        inp = dict(alns=rows_u32(rows, 12).reshape(-1), chain_index=cidx, read_index=csr(lens, first=11 * variant), bounds=bounds)
        outs = dict(hits=rows_u32(want["hits"], 8).reshape(-1), hit_index=want["hit_index"].astype(U64))
        scal = dict(want["report"], rc=0)
        return Data(inp, outs, scal, dict(Q=4, R=2, hit_cap=H))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.SelectReport()
        params = _lib.SelectParams(**fm_select_model.params_of())
        rc = lib.kiss_hip_fmi_select_dev(ctx, VP(p["alns"]), VP(p["chain_index"]), VP(p["read_index"]), host["Q"], 1, VP(p["bounds"]),
                                         host["R"], ctypes.byref(params), VP(p["hits"]), VP(p["hit_index"]), host["hit_cap"],
                                         ctypes.byref(rep), VP(stream))
        scal = report_of(rep, fm_select_model.REPORT_COUNTS)
        scal["rc"] = rc
        return scal


PAIR_COUNTS = ([(3, 2), (0, 4), (70, 5), (2, 2)], [(2, 2), (70, 5), (0, 4), (3, 2)])


@functools.lru_cache(maxsize=None)
def mates_case(variant):
    """four pairs of mates with their hits and alignments (tests/fm_rescue_model.py: random_case), two records of the text"""
    rng = np.random.default_rng(130 + variant)
    return fm_rescue_model.random_case(rng, PAIR_COUNTS[variant], 2000, nrefs=2, extra=1, ins_max=50)


class Pair(Case):
    entry = "kiss_hip_fmi_pair_dev"

    def make(self, variant):
        c = mates_case(variant)
        want = fm_pair_model.pair(c["hits"], c["hit_index"], c["alns"])
        assert want["report"]["proper"] >= 1 and want["report"]["concordant"] >= 2
        inp = dict(hits=rows_u32(c["hits"], 8).reshape(-1), hit_index=np.asarray(c["hit_index"], U64),
                   alns=rows_u32(c["alns"], 12).reshape(-1))
        scal = dict(want["report"], rc=0)
        return Data(inp, dict(pairs=rows_u32(want["pairs"], 10).reshape(-1)), scal, dict(Q=8, aln_count=len(c["alns"])))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.PairReport()
        params = _lib.PairParams(**fm_pair_model.params_of())
        rc = lib.kiss_hip_fmi_pair_dev(ctx, VP(p["hits"]), VP(p["hit_index"]), host["Q"], VP(p["alns"]), host["aln_count"],
                                       ctypes.byref(params), VP(p["pairs"]), ctypes.byref(rep), VP(stream))
        scal = report_of(rep, fm_pair_model.REPORT_COUNTS)
        scal["rc"] = rc
        return scal


class Rescue(Case):
    entry = "kiss_hip_fmi_rescue_dev"
    PARAMS = dict(ins_max=400, max_width=100)

    def make(self, variant):
        c = mates_case(variant)
        n = 3000
        bounds = np.array([0, 1500 - 100 * variant, n], U64)
        pairs = np.zeros((4, 10), np.int64)  # flags 0: not proper, every pair is planned
        pairs[:, 4] = 9 + variant            # (only flags is read)
        want = fm_rescue_model.plan(pairs, c["hits"], c["hit_index"], c["alns"], c["lens"], n, bounds, **self.PARAMS)
        C = want["report"]["chains"]
        assert C >= 20 and want["report"]["split"] > 0
        inp = dict(pairs=rows_u32(pairs, 10).reshape(-1), hits=rows_u32(c["hits"], 8).reshape(-1),
                   hit_index=np.asarray(c["hit_index"], U64), alns=rows_u32(c["alns"], 12).reshape(-1),
                   read_index=csr(c["lens"], first=5 * variant), bounds=bounds)
        outs = dict(chains=rows_u32(want["chains"], 6).reshape(-1), chain_index=want["chain_index"].astype(U64),
                    origin=want["origin"].astype(U32))
        scal = dict(want["report"], rc=0)
        return Data(inp, outs, scal, dict(Q=8, aln_count=len(c["alns"]), n=n, R=2, cap=C))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.RescueReport()
        params = _lib.RescueParams(**fm_rescue_model.params_of(**self.PARAMS))
        rc = lib.kiss_hip_fmi_rescue_dev(ctx, VP(p["pairs"]), VP(p["hits"]), VP(p["hit_index"]), host["Q"], VP(p["alns"]),
                                         host["aln_count"], VP(p["read_index"]), host["n"], VP(p["bounds"]), host["R"],
                                         ctypes.byref(params), VP(p["chains"]), VP(p["chain_index"]), VP(p["origin"]), host["cap"],
                                         ctypes.byref(rep), VP(stream))
        scal = report_of(rep, fm_rescue_model.REPORT_COUNTS)
        scal["rc"] = rc
        return scal


class Merge(Case):
    entry = "kiss_hip_fmi_aln_merge_dev"

    def make(self, variant):
        rng = np.random.default_rng(140 + variant)
        sizes_a, sizes_b = ([3, 0, 70, 2], [1, 66, 0, 2]) if not variant else ([2, 70, 0, 3], [2, 0, 66, 1])
        ia, ib = csr(sizes_a, first=2 + variant), csr(sizes_b, first=variant)
        A = rng.integers(0, 1 << 32, (sum(sizes_a), 12), dtype=np.int64)
        B = rng.integers(0, 1 << 32, (sum(sizes_b), 12), dtype=np.int64)
        # (the totals of the ops are fixed so that the decoy has the shapes of the real input)
        na, nb = rng.permutation(np.arange(A.shape[0]) % 5), rng.permutation(np.arange(B.shape[0]) % 5)
        oa, ob = csr(na), csr(nb)
        ca = rng.integers(0, 1 << 32, int(oa[-1]), dtype=np.int64).astype(U32)
        cb = rng.integers(0, 1 << 32, int(ob[-1]), dtype=np.int64).astype(U32)
        want = fm_rescue_model.merge(A, ia, B, ib, ca, oa, cb, ob)
        C, O = want["alignments"].shape[0], int(want["cigar"].size)
        inp = dict(alns_a=rows_u32(A, 12).reshape(-1), chain_index_a=ia, cigar_a=ca, cigar_index_a=oa, alns_b=rows_u32(B, 12).reshape(-1),
                   chain_index_b=ib, cigar_b=cb, cigar_index_b=ob)
        outs = dict(alns=rows_u32(want["alignments"], 12).reshape(-1), chain_index=want["chain_index"].astype(U64),
                    source=want["source"].astype(U32), cigar=want["cigar"].astype(U32), cigar_index=want["cigar_index"].astype(U64))
        scal = dict(rc=0, V=4, alignments_a=A.shape[0], alignments_b=B.shape[0], alignments=C, cigar_ops=O)
        return Data(inp, outs, scal, dict(V=4, aln_cap=C, cigar_cap=O))

    def call(self, lib, ctx, p, host, stream):
        rep = _lib.MergeReport()
        rc = lib.kiss_hip_fmi_aln_merge_dev(ctx, VP(p["alns_a"]), VP(p["chain_index_a"]), VP(p["cigar_a"]), VP(p["cigar_index_a"]),
                                            VP(p["alns_b"]), VP(p["chain_index_b"]), VP(p["cigar_b"]), VP(p["cigar_index_b"]), host["V"],
                                            VP(p["alns"]), host["aln_cap"], VP(p["chain_index"]), VP(p["source"]), VP(p["cigar"]),
                                            VP(p["cigar_index"]), host["cigar_cap"], ctypes.byref(rep), VP(stream))
        scal = report_of(rep, ("V", "alignments_a", "alignments_b", "alignments", "cigar_ops"))
        scal["rc"] = rc
        return scal


def small(case):
    case.in_stream_test = False
    return case


ALGO_PS, ALGO_PD = _lib.ALGO_PARALLEL_SORTING, _lib.ALGO_PREFIX_DOUBLING
CASES = [
    SortDna("n20003_k32", n=20003, k=32, algo=ALGO_PS),
    SortDna("n4099_k256", n=4099, k=256, algo=ALGO_PS),
    SortDna("n20003_exact_ps", n=20003, k=K_UNBOUNDED, algo=ALGO_PS),
    SortDna("n20003_exact_pd", n=20003, k=K_UNBOUNDED, algo=ALGO_PD),
    small(SortDna("n1", n=1, k=256, algo=ALGO_PS)),
    small(SortDna("n33_exact", n=33, k=K_UNBOUNDED, algo=ALGO_PS)),
    SortU8("english_n4099", kind="english", n=4099),
    SortU8("two_values_n4099_the_dna_path", kind="00_ff", n=4099),
    small(SortU8("english_n33", kind="english", n=33)),
    small(SortU8("english_n1", kind="english", n=1)),
    VerifySa("n4099_k256_damaged", n=4099, k=256, damage=True),
    VerifySa("n20003_exact_damaged", n=20003, k=K_UNBOUNDED, damage=True),
    small(VerifySa("n20003_exact", n=20003, k=K_UNBOUNDED)),
    small(VerifySa("n33_exact_damaged", n=33, k=K_UNBOUNDED, damage=True)),
    small(VerifySa("n1", n=1, k=256)),
    LcpDna("n4099", n=4099),
    small(LcpDna("n33", n=33)),
    small(LcpDna("n1", n=1)),
    LcpU8("n4099", n=4099),
    small(LcpU8("n33", n=33)),
    small(LcpU8("n1", n=1)),
    ParseText("fasta_4099_bytes", bytes=4099),
    ParseText("plain_20003_bytes", bytes=20003, plain=True),
    FmBuild("n4099", n=4099),
    small(FmBuild("n33", n=33)),
    small(FmBuild("n1", n=1)),
    FmBuildEx("n20003_intv7_lookup3", n=20003, sa_intv=7, lookup_len=3),
    small(FmBuildEx("n33_intv1_lookup2", n=33, sa_intv=1, lookup_len=2)),
    FmQuery("n4099", n=4099),
    FmQueryEx("n4099_intv7_lookup3", n=4099, sa_intv=7, lookup_len=3),
    FmQueryEx("n4099_intv1_lookup2_stop3", n=4099, sa_intv=1, lookup_len=2, stop_cnt=3, L=12),
    FmQueryMm("n4099_e2", n=4099),
    Fm8Build("english_n4099", n=4099),
    small(Fm8Build("english_n33_intv1", n=33, sa_intv=1)),
    small(Fm8Build("english_n1", n=1)),
    Fm8Query("english_n4099", n=4099),
    Seeds("n2000_both_strands", n=2000, both=True),
    Seeds("n2000_forward", n=2000, both=False),
    Chain("five_virtual_reads"),
    Align("n2000_both_strands", n=2000),
    Select("both_strands_bounds"),
    Pair("four_pairs"),
    Rescue("four_pairs_bounds"),
    Merge("with_ops"),
]
