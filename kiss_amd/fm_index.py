"""Host-side mirror of biovoltron::FMIndex<SA_INTV, uint32_t, KISS1Sorter<uint32_t>>{.LOOKUP_LEN}
(reference include/biovoltron/algo/align/exact_match/fm_index.hpp).  The defaults, SA_INTV = 4 and LOOKUP_LEN = 0, are
the instantiation of the reference CLI (include/command/fmindex_build.hpp:27-29 and fmindex_query.hpp:26-28) and run
through the original entry points; FMIndex(sa_intv=1..32, lookup_len=0..14) runs through the kiss_hip_fmi_*_ex_* ones.

Same member names and meaning: build(ref), save(path) / load(path) in the reference's `.fmi`
byte layout (fm_index.hpp:591-646), get_range(seed), get_offsets(beg, end), plus
query_batch(patterns) which replaces the per-pattern loop of fmindex_query_main
(include/command/fmindex_query.hpp:79-95).

All arithmetic runs in libkiss_hip.so through its C ABI; torch only owns the device buffers.
There is no CPU path.
"""
import ctypes
import struct
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._frame import read_batch, read_list, record_view
from .sorter import Context, K_UNBOUNDED, _check

SA_INTV = 4          # fmindex_build.hpp:27
MAX_SA_INTV, MAX_LOOKUP_LEN = 32, 14  # KISS_HIP_FMI_MAX_SA_INTV / KISS_HIP_FMI_MAX_LOOKUP_LEN
MAX_MISMATCHES = 3   # KISS_HIP_FMI_MAX_MISMATCHES
SORT_LEN = 32        # FMIndex::build sorts with k = 32 whatever the CLI flags say (fm_index.hpp:384-386)
OCC1_INTV, OCC2_INTV, B_OCC_INTV = 256, 16, 64


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kiss_amd.FMIndex needs a HIP device (no CPU fallback)")
    return torch


def _check_params(sa_intv, lookup_len):
    if not 1 <= sa_intv <= MAX_SA_INTV:
        raise ValueError("sa_intv must be in 1..%d, got %d" % (MAX_SA_INTV, sa_intv))
    if not 0 <= lookup_len <= MAX_LOOKUP_LEN:
        raise ValueError("lookup_len must be in 0..%d, got %d" % (MAX_LOOKUP_LEN, lookup_len))


@dataclass
class _Aligned:
    """what _align_dev leaves on the device for the stages after it (select, insert, pair, rescue, MD)"""
    lib: object          # the library that serves the index
    ctx: object          # the context the align call ran on
    d_text: object       # the text, its length n
    n: int
    d_reads: object      # the reads, their index (Q + 1) and, on the host, their lengths
    d_ridx: object
    Q: int
    lens: object
    d_cidx: object       # the chain index (V + 1) and the C alignments of the chains
    d_alns: object
    C: int
    al: dict             # all of align_dev's output: the ops and their index, the report
    align_params: object
    keep: tuple          # the outputs of the seeds and the chain call, which the tensors above are part of


class FMIndex:
    def __init__(self, device=0, sa_intv=SA_INTV, lookup_len=0, hooks=None):
        """hooks (here, on load and on from_bytes) is for the tests and the measuring tools only: True serves this index
        from libkiss_hip_hooks.so, the build with the A-B switches; None, the default, from the library of the process."""
        _check_params(int(sa_intv), int(lookup_len))
        self.device = int(device)
        self._hooks = hooks  # which build of the library serves this index (_lib.load): None = the process default
        self.sa_intv = int(sa_intv)
        self.lookup_len = int(lookup_len)
        self.N = 0
        self.cnt = np.zeros(4, np.uint32)
        self.pri = 0
        # torch tensors on the GPU; b / b_occ stay None when sa_intv == 1 (the reference keeps no bit-vector)
        self.bwt = self.occ1 = self.occ2 = self.sa = self.b = self.b_occ = self.lookup = None
        self._ctx = None
        # the index was built from the EXACT suffix array: what query_mismatch needs for positions
        self.exact_sa = False

    @property
    def _classic(self):
        """the CLI's instantiation, served by the original entry points"""
        return self.sa_intv == SA_INTV and self.lookup_len == 0

    # ---- sizes of the .fmi arrays for an SA of N entries -------------------------------------------
    @staticmethod
    def _sizes(N, sa_intv=SA_INTV, lookup_len=0):
        return {
            "bwt": (N + 3) // 4,                      # bytes
            "occ1": (N // OCC1_INTV + 1) * 4,          # u32
            "occ2": (N // OCC2_INTV + 1) * 4,          # u8
            "sa": (N + sa_intv - 1) // sa_intv,        # u32
            "lookup": 4 ** lookup_len + 1,             # u32
            "b": (N + 63) // 64 if sa_intv != 1 else 0,        # u64
            "b_occ": N // B_OCC_INTV + 1 if sa_intv != 1 else 0,  # u32
        }

    def _alloc(self, N):
        torch = _torch()
        dev = torch.device("cuda", self.device)
        sz = self._sizes(N, self.sa_intv, self.lookup_len)
        self.N = N
        self.bwt = torch.zeros(sz["bwt"] + 8, dtype=torch.uint8, device=dev)
        self.occ1 = torch.zeros(sz["occ1"], dtype=torch.int32, device=dev)
        self.occ2 = torch.zeros(sz["occ2"], dtype=torch.uint8, device=dev)
        self.sa = torch.zeros(sz["sa"], dtype=torch.int32, device=dev)
        self.lookup = torch.zeros(sz["lookup"], dtype=torch.int32, device=dev)
        if self.sa_intv != 1:
            self.b = torch.zeros(sz["b"] + 1, dtype=torch.int64, device=dev)
            self.b_occ = torch.zeros(sz["b_occ"], dtype=torch.int32, device=dev)
        else:
            self.b = self.b_occ = None

    def _context(self, max_n):
        if self._ctx is None or self._ctx.max_n < max_n:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = Context(max_n=max(max_n, 1 << 20), device=self.device, hooks=self._hooks)
        return self._ctx

    def _context_to_sort(self, ctx, count):
        """ctx, or a context whose LMS arrays (0.32 max_n entries), where a call sorts its items, hold `count` of them"""
        if count > 0.3 * ctx.max_n:
            ctx = self._context(min(_lib.MAX_N, int(3.3 * count) + (1 << 20)))
        return ctx

    def _text_dev(self, text):
        """the text, a uint8 array or a tensor, on the device (one element when it is empty: no NULL) -> tensor, length"""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(text, torch.Tensor):
            d_text = text.to(device=dev, dtype=torch.uint8).contiguous().reshape(-1)
        else:
            arr = np.ascontiguousarray(text, dtype=np.uint8).ravel()
            d_text = torch.from_numpy(arr).to(dev) if arr.size else torch.zeros(0, dtype=torch.uint8, device=dev)
        n = int(d_text.numel())
        return (d_text if n else torch.zeros(1, dtype=torch.uint8, device=dev)), n

    # ---- build (fm_index.hpp:379-451) ------------------------------------------------------------------
    def build(self, ref, sa=None, exact=False, exact_sa=False):
        """ref: uint8 array with values 0..3.  Sorts with k = 32 (like the reference) unless `sa` is given;
        exact=True sorts in exact order instead (K_UNBOUNDED: what the positions of query_mismatch need; same .fmi
        layout).  exact_sa: the caller's word that a given `sa` is the exact suffix array.
        ref / sa may also be device tensors of this device (uint8 / int32 holding the u32 values): used in place."""
        if exact and sa is not None:
            raise ValueError("exact=True sorts the text itself; with sa= say exact_sa=True instead")
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(ref, torch.Tensor) and ref.device == dev:
            d_S = ref.contiguous()
        else:
            d_S = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.uint8)).to(dev)
        n = d_S.numel()
        ctx = self._context(n)
        if sa is None:
            d_SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
            ctx.suffix_sort_dev(d_S.data_ptr(), n, d_SA.data_ptr(), k=K_UNBOUNDED if exact else SORT_LEN)
        elif isinstance(sa, torch.Tensor) and sa.device == dev:
            d_SA = sa.contiguous()
            if d_SA.numel() != n + 1 or d_SA.element_size() != 4:
                raise ValueError("sa must hold n + 1 32-bit entries")
        else:
            d_SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
            d_SA.copy_(torch.from_numpy(np.ascontiguousarray(sa, dtype=np.uint32).view(np.int32)))
        self._alloc(n + 1)
        cnt = (ctypes.c_uint32 * 4)()
        pri = ctypes.c_uint32()
        lib = _lib.load(self._hooks)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        if self._classic:
            _check(lib.kiss_hip_fmi_build_dev(ctx._ctx, ctypes.c_void_p(d_S.data_ptr()), n,
                                              ctypes.c_void_p(d_SA.data_ptr()), SA_INTV,
                                              ptr(self.bwt), ptr(self.occ1), ptr(self.occ2), ptr(self.sa), ptr(self.b),
                                              ptr(self.b_occ), ctypes.byref(cnt), ctypes.byref(pri), None),
                   "kiss_hip_fmi_build_dev", ctx._ctx)
            self.lookup.copy_(torch.tensor([0, n + 1], dtype=torch.int64).to(torch.int32))  # LOOKUP_LEN = 0: {0, N}
        else:
            _check(lib.kiss_hip_fmi_build_ex_dev(ctx._ctx, ctypes.c_void_p(d_S.data_ptr()), n,
                                                 ctypes.c_void_p(d_SA.data_ptr()), self.sa_intv, self.lookup_len,
                                                 ptr(self.bwt), ptr(self.occ1), ptr(self.occ2), ptr(self.sa), ptr(self.b),
                                                 ptr(self.b_occ), ptr(self.lookup), ctypes.byref(cnt), ctypes.byref(pri),
                                                 None),
                   "kiss_hip_fmi_build_ex_dev", ctx._ctx)
        self.cnt = np.array(list(cnt), dtype=np.uint32)
        self.pri = int(pri.value)
        self.exact_sa = bool(exact or (sa is not None and exact_sa))
        return self

    # ---- .fmi serialisation (fm_index.hpp:591-646; Serializer: u64 count + raw bytes, nothing when empty) -----
    # order: cnt, pri, bwt, occ1, occ2, sa_, lookup_, then b_ and b_occ_ only if SA_INTV != 1; no header (SA_INTV is a
    # template parameter of the reference, LOOKUP_LEN follows from the lookup_ count)
    def to_bytes(self):
        sz = self._sizes(self.N, self.sa_intv, self.lookup_len)
        N = self.N
        out = [self.cnt.astype("<u4").tobytes(), struct.pack("<I", self.pri)]

        def vec(count, raw):
            if count:
                out.append(struct.pack("<Q", count))
                out.append(raw)
        vec(N, self.bwt[:sz["bwt"]].cpu().numpy().tobytes())
        vec(sz["occ1"] // 4, self.occ1.cpu().numpy().view(np.uint32).astype("<u4").tobytes())
        vec(sz["occ2"] // 4, self.occ2.cpu().numpy().tobytes())
        vec(sz["sa"], self.sa.cpu().numpy().view(np.uint32).astype("<u4").tobytes())
        vec(sz["lookup"], self.lookup.cpu().numpy().view(np.uint32).astype("<u4").tobytes())  # (fm_index.hpp:238-270)
        if self.sa_intv != 1:
            vec(N, self.b[:sz["b"]].cpu().numpy().view(np.uint64).astype("<u8").tobytes())
            vec(sz["b_occ"], self.b_occ.cpu().numpy().view(np.uint32).astype("<u4").tobytes())
        return b"".join(out)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, buf, device=0, sa_intv=SA_INTV, exact_sa=False, hooks=None):
        """the file does not record SA_INTV: the caller names it, and a file whose vector counts do not fit it is
        rejected; LOOKUP_LEN is read from the lookup_ count (4^L + 1).  Nor does it record the order of the suffix array it
        was built from: exact_sa is the caller's word that it was the exact one."""
        torch = _torch()
        _check_params(int(sa_intv), 0)
        mv = memoryview(buf)
        cnt = np.frombuffer(mv[:16], dtype="<u4").astype(np.uint32)
        pri = struct.unpack_from("<I", mv, 16)[0]
        off = 20

        def vec(elem_bytes_of_count):
            nonlocal off
            if off + 8 > len(mv):
                raise ValueError("truncated .fmi")
            count = struct.unpack_from("<Q", mv, off)[0]
            off += 8
            nbytes = elem_bytes_of_count(count)
            if off + nbytes > len(mv):
                raise ValueError("truncated .fmi")
            raw = bytes(mv[off:off + nbytes])
            off += nbytes
            return count, raw
        N, bwt = vec(lambda c: (c + 3) // 4)
        c_occ1, occ1 = vec(lambda c: c * 16)
        c_occ2, occ2 = vec(lambda c: c * 4)
        c_sa, sa = vec(lambda c: c * 4)
        c_lookup, lookup = vec(lambda c: c * 4)
        lookup_len = next((L for L in range(MAX_LOOKUP_LEN + 1) if 4 ** L + 1 == c_lookup), None)
        if lookup_len is None:
            raise ValueError("lookup_ has %d entries, not 4^L + 1 for any L in 0..%d" % (c_lookup, MAX_LOOKUP_LEN))
        sz = cls._sizes(N, sa_intv, lookup_len)
        if c_occ1 * 4 != sz["occ1"] or c_occ2 * 4 != sz["occ2"]:
            raise ValueError("occ sizes of the .fmi do not fit N = %d" % N)
        if c_sa != sz["sa"]:
            raise ValueError("sa_ has %d entries; SA_INTV = %d needs %d" % (c_sa, sa_intv, sz["sa"]))
        b = b_occ = None
        if sa_intv != 1:
            c_b, b = vec(lambda c: ((c + 63) // 64) * 8)
            c_bocc, b_occ = vec(lambda c: c * 4)
            if c_b != N or c_bocc != sz["b_occ"]:
                raise ValueError("b_ / b_occ_ sizes of the .fmi do not fit N = %d" % N)
        if off != len(mv):
            raise ValueError("trailing bytes in .fmi (the reference asserts EOF, fm_index.hpp:642)")
        self = cls(device, sa_intv=sa_intv, lookup_len=lookup_len, hooks=hooks)
        self.exact_sa = bool(exact_sa)
        self.cnt = cnt
        self.pri = pri
        self._alloc(N)
        dev = self.bwt.device

        def put(dst, raw, dtype):
            a = np.frombuffer(raw, dtype=dtype).copy()
            t = torch.from_numpy(a.view({np.dtype("<u4"): np.int32, np.dtype("<u8"): np.int64,
                                         np.dtype("u1"): np.uint8}[np.dtype(dtype)]))
            dst[:t.numel()].copy_(t.to(dev))
        put(self.bwt, bwt, "u1")
        put(self.occ1, occ1, "<u4")
        put(self.occ2, occ2, "u1")
        put(self.sa, sa, "<u4")
        put(self.lookup, lookup, "<u4")
        if sa_intv != 1:
            put(self.b, b, "<u8")
            put(self.b_occ, b_occ, "<u4")
        return self

    @classmethod
    def load(cls, path, device=0, sa_intv=SA_INTV, exact_sa=False, hooks=None):
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), device, sa_intv, exact_sa, hooks)

    # ---- queries -------------------------------------------------------------------------------------------
    def _view(self):
        v = _lib.FmiView()
        v.n_sa = self.N
        for c in range(4):
            v.cnt[c] = int(self.cnt[c])
        v.pri = self.pri
        v.sa_intv = self.sa_intv
        v.bwt = self.bwt.data_ptr()
        v.occ1 = self.occ1.data_ptr()
        v.occ2 = self.occ2.data_ptr()
        v.sa = self.sa.data_ptr()
        v.b = self.b.data_ptr() if self.b is not None else None
        v.b_occ = self.b_occ.data_ptr() if self.b_occ is not None else None
        return v

    def query_batch(self, patterns, want_offsets=True, d_patterns=None, keep_on_device=False, stop_cnt=0, want_offs=False):
        """patterns: (Q, L) uint8 array with values 0..3 (host) or a device tensor via d_patterns.
        Returns dict(beg, end, total_hits, checksum[, offsets, offsets_index][, offs]); keep_on_device: beg / end (and
        offs) stay device tensors (int32 holding the u32 values) instead of being copied to the host.
        stop_cnt: get_range's early stop (0: none; 0xFFFFFFFF also never stops, stop_cnt + 1 wraps in u32);
        want_offs: also get_range's third value, the characters left unmatched per pattern."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        stop_cnt = int(stop_cnt)
        if not 0 <= stop_cnt <= 0xFFFFFFFF:
            raise ValueError("stop_cnt is a u32")
        if d_patterns is None:
            patterns = np.ascontiguousarray(patterns, dtype=np.uint8)
            d_patterns = torch.from_numpy(patterns).to(dev)
        Q, L = int(d_patterns.shape[0]), int(d_patterns.shape[1])
        ctx = self._context(max(self.N, 4 * Q))
        beg = torch.empty(Q, dtype=torch.int32, device=dev)
        end = torch.empty(Q, dtype=torch.int32, device=dev)
        offs = torch.empty(Q, dtype=torch.int32, device=dev) if want_offs else None
        tot = ctypes.c_uint64()
        chk = ctypes.c_uint64()
        lib = _lib.load(self._hooks)
        view = self._view()
        if self._classic and stop_cnt == 0 and not want_offs:
            def call(offsets, index, cap):
                _check(lib.kiss_hip_fmi_query_batch_dev(ctx._ctx, ctypes.byref(view), ctypes.c_void_p(d_patterns.data_ptr()),
                                                        L, Q, ctypes.c_void_p(beg.data_ptr()),
                                                        ctypes.c_void_p(end.data_ptr()), ctypes.byref(tot),
                                                        ctypes.byref(chk), offsets, index, cap, None),
                       "kiss_hip_fmi_query_batch_dev", ctx._ctx)
        else:
            vex = _lib.FmiViewEx()
            vex.base = view
            vex.lookup_len = self.lookup_len
            vex.lookup = self.lookup.data_ptr()

            def call(offsets, index, cap):
                _check(lib.kiss_hip_fmi_query_ex_dev(ctx._ctx, ctypes.byref(vex), ctypes.c_void_p(d_patterns.data_ptr()),
                                                     L, Q, stop_cnt, ctypes.c_void_p(beg.data_ptr()),
                                                     ctypes.c_void_p(end.data_ptr()),
                                                     ctypes.c_void_p(offs.data_ptr() if offs is not None else None),
                                                     ctypes.byref(tot), ctypes.byref(chk), offsets, index, cap, None),
                       "kiss_hip_fmi_query_ex_dev", ctx._ctx)
        res = {}
        # first pass sizes the output; the library needs a capacity, so run ranges once to learn it
        call(None, None, 0)
        if want_offsets:
            cap = int(tot.value)
            offsets = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
            index = torch.empty(Q + 1, dtype=torch.int64, device=dev)
            call(ctypes.c_void_p(offsets.data_ptr()), ctypes.c_void_p(index.data_ptr()), cap)
            res["offsets"] = offsets[:cap].cpu().numpy().view(np.uint32)
            res["offsets_index"] = index.cpu().numpy().view(np.uint64)
        if keep_on_device:
            res["beg"], res["end"] = beg, end
            if offs is not None:
                res["offs"] = offs
        else:
            res["beg"] = beg.cpu().numpy().view(np.uint32)
            res["end"] = end.cpu().numpy().view(np.uint32)
            if offs is not None:
                res["offs"] = offs.cpu().numpy().view(np.uint32)
        res["total_hits"] = int(tot.value)
        res["checksum"] = int(chk.value)
        return res

    def get_range(self, seed, stop_cnt=0, with_offset=False):
        """(beg, end) of one pattern (fm_index.hpp:553-584); with_offset: (beg, end, offset), the reference's array"""
        r = self.query_batch(np.asarray(seed, dtype=np.uint8)[None, :], want_offsets=False, stop_cnt=stop_cnt,
                             want_offs=with_offset)
        if with_offset:
            return int(r["beg"][0]), int(r["end"][0]), int(r["offs"][0])
        return int(r["beg"][0]), int(r["end"][0])

    def get_offsets_of(self, seed):
        """hit positions of one pattern in the reference's get_offsets order (fm_index.hpp:453-501)."""
        r = self.query_batch(np.asarray(seed, dtype=np.uint8)[None, :], want_offsets=True)
        return r["offsets"]

    # ---- search with mismatches (kiss_hip_fmi_query_mm_dev; no reference counterpart) --------------------------------
    def query_mismatch(self, patterns, max_mismatches, want_positions=True, d_patterns=None):
        """Every text position whose Hamming distance to a pattern is at most max_mismatches (0..3; substitutions only).
        patterns: (Q, L) uint8, used & 3 (host), or a device tensor via d_patterns.  Returns dict(counts (Q, e + 1):
        hits by number of mismatches, hits_by_mismatch, total_hits, checksum, report) and, with want_positions,
        positions / mismatches / index in CSR layout (index: Q + 1 u64), ascending position inside a pattern.
        Counts are defined for L <= the order of the build (32 by default, any L after build(exact=True)); positions
        only on an index built from the exact suffix array.  With positions the batch is searched twice, as the C
        interface has it: once for the counts, which size the output and say where to cut a batch that has more hits
        than one call sorts, then part by part; `report` sums the calls of the second kind (`calls` of them) and gives the
        first one's time as `ms_counts`."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        e = int(max_mismatches)
        if not 0 <= e <= MAX_MISMATCHES:
            raise ValueError("max_mismatches must be in 0..%d, got %d" % (MAX_MISMATCHES, e))
        if want_positions and not self.exact_sa:
            raise ValueError("positions of a search with mismatches need an index built from the exact suffix array: "
                             "build(ref, exact=True), or exact_sa=True on build(sa=...) / load / from_bytes")
        if d_patterns is None:
            d_patterns = torch.from_numpy(np.ascontiguousarray(patterns, dtype=np.uint8)).to(dev)
        d_patterns = d_patterns.contiguous()
        Q, L = int(d_patterns.shape[0]), int(d_patterns.shape[1])
        if L == 0:
            raise ValueError("patterns of length 0")
        lib = _lib.load(self._hooks)
        view = self._view()
        counts = torch.zeros((Q, e + 1), dtype=torch.int32, device=dev)
        hits = [0, 0, 0, 0]
        acc = {"ranges": 0, "lf_pairs": 0, "walk_failures": 0, "checksum": 0, "ms_total": 0.0, "ms_search": 0.0,
               "ms_locate": 0.0, "ms_sort": 0.0, "calls": 0, "ms_counts": 0.0}
        pos_parts, mm_parts, sizes = [], [], []

        def add(rep):
            for k in acc:
                if k not in ("calls", "ms_counts"):
                    acc[k] += getattr(rep, k)
            acc["calls"] += 1
            for j in range(4):
                hits[j] += int(rep.hits[j])

        def locate(lo, hi, total):
            """positions of the patterns [lo, hi), which have `total` hits -> the status of the call"""
            q = hi - lo
            ctx = self._ctx
            positions = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            mism = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
            index = torch.empty(q + 1, dtype=torch.int64, device=dev)
            rep = _lib.FmiMmReport()
            rc = lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), ctypes.c_void_p(d_patterns.data_ptr() + lo * L), L, q,
                                               e, ctypes.c_void_p(counts.data_ptr() + lo * (e + 1) * 4),
                                               ctypes.c_void_p(positions.data_ptr()), ctypes.c_void_p(mism.data_ptr()),
                                               ctypes.c_void_p(index.data_ptr()), total, ctypes.byref(rep), None)
            if rc == _lib.KISS_HIP_E_UNSUPPORTED:
                return rc
            if rc == _lib.KISS_HIP_E_INVALID and rep.walk_failures:
                raise _lib.KissHipError(rc, "kiss_hip_fmi_query_mm_dev",
                                        "%d rows reached no sampled row: the index was not built from an exact suffix array "
                                        "(build with exact=True)" % rep.walk_failures)
            _check(rc, "kiss_hip_fmi_query_mm_dev", ctx._ctx)
            add(rep)
            pos_parts.append(positions[:total].cpu().numpy().view(np.uint32))
            mm_parts.append(mism[:total].cpu().numpy())
            sizes.append(np.diff(index.cpu().numpy().view(np.uint64)))
            return rc

        def run():
            """counts of the whole batch first: they size the output and say where to cut the batch so that every part
            has no more hits than one call sorts (the context's per-LMS-suffix arrays, 0.32 max_n entries)"""
            ctx = self._context(max(self.N, 4 * Q))
            rep = _lib.FmiMmReport()
            _check(lib.kiss_hip_fmi_query_mm_dev(ctx._ctx, ctypes.byref(view), ctypes.c_void_p(d_patterns.data_ptr()), L, Q, e,
                                                 ctypes.c_void_p(counts.data_ptr()), None, None, None, 0, ctypes.byref(rep), None),
                   "kiss_hip_fmi_query_mm_dev", ctx._ctx)
            if not want_positions:
                add(rep)
                return
            acc["ms_counts"] = float(rep.ms_total)  # (the rest of the report: the calls that return the positions)
            ends = counts.to(torch.int64).sum(dim=1).cumsum(0).cpu().numpy()  # hits of the patterns [0, q]
            cap = int(0.32 * ctx.max_n)
            parts, lo = [], 0
            while lo < Q:
                before = int(ends[lo - 1]) if lo else 0
                hi = max(int(np.searchsorted(ends, before + cap, side="right")), lo + 1)
                parts.append((lo, hi))
                lo = hi
            while parts:
                lo, hi = parts.pop(0)
                total = int(ends[hi - 1]) - (int(ends[lo - 1]) if lo else 0)
                if locate(lo, hi, total) != _lib.KISS_HIP_E_UNSUPPORTED:
                    continue
                if hi - lo > 1:  # (the context sorts fewer than reckoned with: halve)
                    parts[:0] = [(lo, lo + (hi - lo) // 2), (lo + (hi - lo) // 2, hi)]
                    continue
                self._context(min(_lib.MAX_N, 4 * total + (1 << 20)))  # one pattern with that many hits: a larger context
                _check(locate(lo, hi, total), "kiss_hip_fmi_query_mm_dev", self._ctx._ctx)

        if Q:
            run()
        rep = dict(acc)
        rep.update(Q=Q, L=L, max_mismatches=e, hits=list(hits))
        res = {"counts": counts.cpu().numpy().view(np.uint32), "hits_by_mismatch": hits[:e + 1], "total_hits": sum(hits),
               "checksum": int(acc["checksum"]), "report": rep}
        if want_positions:
            res["positions"] = np.concatenate(pos_parts) if pos_parts else np.zeros(0, np.uint32)
            res["mismatches"] = np.concatenate(mm_parts) if mm_parts else np.zeros(0, np.uint8)
            index = np.zeros(Q + 1, np.uint64)
            if sizes:
                np.cumsum(np.concatenate(sizes), out=index[1:])
            res["index"] = index
        return res

    # ---- maximal exact match seeds (kiss_hip_fmi_seeds_dev; no reference counterpart) -------------------------------
    def seeds(self, reads, min_len=19, max_len=0, max_occ=500, both_strands=False, want_positions=True, want_ms=False):
        """The maximal exact match seeds of a batch of reads (include/kiss_hip.h has the definition).
        reads: a list of uint8 arrays, or (concatenated, index) with read q = concatenated[index[q]:index[q + 1]].  The
        values 0..3 are bases, any other value is no base (N): no seed contains it.  both_strands: virtual read 2 q is read
        q, 2 q + 1 its reverse complement; otherwise virtual read q is read q.
        Returns dict(seeds: structured array (start, len, sa_beg, sa_end), seed_index (V + 1: the seeds of virtual read v
        are seeds[seed_index[v]:seed_index[v + 1]], ascending start), count (sa_end - sa_beg), report) and, with
        want_positions, positions / pos_index in CSR layout over the seeds (ascending inside a seed; seeds with more than
        max_occ occurrences -- 0: no limit -- have an empty segment), with want_ms the matching statistics `ms` (one per
        end, virtual read after virtual read).
        max_len: 0 = no cap.  Seeds are defined for max_len <= the order of the build: 1..32 by default, any value after
        build(exact=True); positions only on an index built from the exact suffix array.  With positions the batch is
        searched twice, as the C interface has it: the first call sizes the output."""
        from .fm_chain import SEED_DTYPE
        d = self._seeds_dev(reads, min_len, max_len, max_occ, both_strands, want_positions, want_ms)
        rep, nseeds = d["rep"], d["nseeds"]
        res = {}
        if want_positions:
            res["positions"] = d["d_pos"][:d["total"]].cpu().numpy().view(np.uint32)
            res["pos_index"] = d["d_pidx"].cpu().numpy().view(np.uint64)
        res["seeds"] = seeds = record_view(d["d_seeds"], nseeds, SEED_DTYPE)
        res["seed_index"] = d["d_sidx"].cpu().numpy().view(np.uint64)
        res["count"] = (seeds["sa_end"] - seeds["sa_beg"]).astype(np.uint32)
        if want_ms:
            res["ms"] = d["d_ms"][:d["bases"]].cpu().numpy().view(np.uint32)
        res["report"] = rep.as_dict()
        return res

    def _seeds_dev(self, reads, min_len, max_len, max_occ, both_strands, want_positions, want_ms):
        """the device half of seeds(): checks, upload and the call(s); the outputs stay on the device (torch tensors)"""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        min_len, max_len, max_occ = int(min_len), int(max_len), int(max_occ)
        if min_len < 1:
            raise ValueError("min_len must be at least 1")
        if max_len < 0 or max_occ < 0 or max(min_len, max_len, max_occ) > 0xFFFFFFFF:
            raise ValueError("min_len, max_len and max_occ are u32 (0: no cap / no limit)")
        if not self.exact_sa:
            if want_positions:
                raise ValueError("positions of seeds need an index built from the exact suffix array: "
                                 "build(ref, exact=True), or exact_sa=True on build(sa=...) / load / from_bytes")
            if max_len == 0 or max_len > SORT_LEN:
                raise ValueError("an index of a suffix array of order %d defines seeds for max_len in 1..%d only "
                                 "(build with exact=True for longer ones)" % (SORT_LEN, SORT_LEN))
        cat, index = read_batch(reads)
        if index.ndim != 1 or index.size < 1:
            raise ValueError("the read index has Q + 1 entries")
        Q = int(index.size) - 1
        if Q and (np.any(index[1:] <= index[:-1]) or int(index[-1]) > cat.size):
            raise ValueError("reads of length 0, or a read index that decreases or points past the reads")
        V = 2 * Q if both_strands else Q
        bases = (int(index[-1]) - int(index[0])) * (2 if both_strands else 1) if Q else 0
        lib = _lib.load(self._hooks)
        vex = _lib.FmiViewEx()
        vex.base = self._view()
        vex.lookup_len = self.lookup_len
        vex.lookup = self.lookup.data_ptr() if self.lookup is not None else None
        vp = ctypes.c_void_p
        d_reads = torch.from_numpy(cat).to(dev) if cat.size else torch.zeros(1, dtype=torch.uint8, device=dev)
        d_index = torch.from_numpy(index.view(np.int64)).to(dev)
        d_ms = torch.zeros(max(bases, 1), dtype=torch.int32, device=dev) if want_ms else None
        d_seeds = torch.zeros((max(bases, 1), 4), dtype=torch.int32, device=dev)
        d_sidx = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        rep = _lib.FmiSeedReport()

        def call(ctx, d_pos, d_pidx, cap):
            return lib.kiss_hip_fmi_seeds_dev(ctx._ctx, ctypes.byref(vex), vp(d_reads.data_ptr()), vp(d_index.data_ptr()), Q,
                                              min_len, max_len, max_occ, 1 if both_strands else 0,
                                              vp(d_ms.data_ptr() if d_ms is not None else None), vp(d_seeds.data_ptr()),
                                              vp(d_sidx.data_ptr()), bases, d_pos, d_pidx, cap, ctypes.byref(rep), None)

        # the ends of a call are scanned in the context's scratch (0.32 max_n entries)
        ctx = self._context(min(_lib.MAX_N, max(self.N, 4 * (bases + 1))))
        _check(call(ctx, None, None, 0), "kiss_hip_fmi_seeds_dev", ctx._ctx)
        out = {"d_seeds": d_seeds, "d_sidx": d_sidx, "d_ms": d_ms, "rep": rep, "V": V, "bases": bases, "total": 0,
               "d_reads": d_reads, "d_ridx": d_index, "Q": Q}
        if want_positions:
            total, nseeds = int(rep.positions), int(rep.seeds)
            ctx = self._context_to_sort(ctx, total)  # (the positions)
            d_pos = torch.zeros(max(total, 1), dtype=torch.int32, device=dev)
            d_pidx = torch.zeros(nseeds + 1, dtype=torch.int64, device=dev)
            rc = call(ctx, vp(d_pos.data_ptr()), vp(d_pidx.data_ptr()), total)
            if rc == _lib.KISS_HIP_E_INVALID and rep.walk_failures:
                raise _lib.KissHipError(rc, "kiss_hip_fmi_seeds_dev",
                                        "%d rows reached no sampled row: the index was not built from an exact suffix array "
                                        "(build with exact=True)" % rep.walk_failures)
            if rc == _lib.KISS_HIP_E_UNSUPPORTED:
                raise _lib.KissHipError(rc, "kiss_hip_fmi_seeds_dev",
                                        "%d positions are more than one call sorts: split the batch" % total)
            _check(rc, "kiss_hip_fmi_seeds_dev", ctx._ctx)
            out.update(d_pos=d_pos, d_pidx=d_pidx, total=total)
        out["nseeds"] = int(rep.seeds)
        out["ctx"] = ctx
        return out

    # ---- the seeds chained into candidate loci (kiss_hip_fmi_chain_dev; no reference counterpart) --------------------
    def chains(self, reads, min_len=19, max_len=0, max_occ=500, both_strands=False, want_anchors=False, **params):
        """The seeds of every read chained into candidate loci (include/kiss_hip.h has the definition): the seeds call and
        the chain call, with the seeds and their positions staying on the device.  reads and the seed parameters as in
        seeds(); params: max_gap (5000), band (500), gap_cost (2), max_lookback (64; 0: no bound), min_score (40).
        Returns dict(chains: structured array (score, anchors, rbeg, rend, tbeg, tend), chain_index (V + 1: the chains of
        virtual read v are chains[chain_index[v]:chain_index[v + 1]], ascending tbeg), report, seed_report) and, with
        want_anchors, anchors (rstart, tpos, len) / anchor_index in CSR layout over the chains, root to end.
        Needs an index built from the exact suffix array, as seeds(want_positions=True) does."""
        from .fm_chain import chain_params, chain_dev, chain_arrays
        p = chain_params(**params)
        d = self._seeds_dev(reads, min_len, max_len, max_occ, both_strands, True, False)
        ctx = self._context_to_sort(d["ctx"], d["total"])  # (the anchors are sorted where the positions were)
        out = chain_dev(_lib.load(self._hooks), ctx, self.device, d["d_seeds"], d["d_sidx"], d["V"], d["d_pos"], d["d_pidx"], p,
                        want_anchors)
        res = chain_arrays(out, want_anchors)
        res["seed_report"] = d["rep"].as_dict()
        return res

    # ---- the chains aligned to the text (kiss_hip_fmi_align_dev; no reference counterpart) ----------------------------
    def align(self, reads, text, min_len=19, max_len=0, max_occ=500, both_strands=False, chain_params=None, want_cigar=True,
              **params):
        """Seeds, chains and the banded affine-gap local alignment of every chain to the text (include/kiss_hip.h has the
        definition), with the reads, the seeds and the chains staying on the device.  text: the bases the index was built
        from (the index does not keep them), a uint8 array or a device tensor; reads and the seed parameters as in seeds();
        chain_params: a dict of the parameters of chains(); params: match (1), mismatch (4), gap_open (6), gap_extend (1),
        band (32).  Returns what chains() returns plus alignments (structured array: score, flags, rbeg, rend, tbeg, tend,
        matches, mismatches, ins, del, gaps, band; alignment c belongs to chain c), align_report and, with want_cigar,
        cigar (u32 ops len << 4 | op, op 0 M, 1 I, 2 D) / cigar_index in CSR layout over the chains."""
        res, _ = self._align_dev(reads, text, min_len, max_len, max_occ, both_strands, chain_params, want_cigar, params)
        return res

    def _align_dev(self, reads, text, min_len, max_len, max_occ, both_strands, chain_params, want_cigar, params):
        """align(): -> (its result, the device tensors a later stage reads: reads, read index, chain index, alignments)"""
        from .fm_align import align_arrays, align_dev, align_params
        from .fm_chain import chain_params as make_chain_params, chain_dev, chain_arrays
        _torch()  # (no device: said before anything else)
        p = align_params(**params)
        cp = make_chain_params(**(chain_params or {}))
        d_text, n = self._text_dev(text)
        d = self._seeds_dev(reads, min_len, max_len, max_occ, both_strands, True, False)
        ctx = self._context_to_sort(d["ctx"], d["total"])  # (the anchors are sorted where the positions were)
        lib = _lib.load(self._hooks)
        out = chain_dev(lib, ctx, self.device, d["d_seeds"], d["d_sidx"], d["V"], d["d_pos"], d["d_pidx"], cp, False)
        res = chain_arrays(out, False)
        res["seed_report"] = d["rep"].as_dict()
        C = int(out["rep"].chains)
        ridx = d["d_ridx"].cpu().numpy().view(np.uint64)
        lens = (ridx[1:] - ridx[:-1]).astype(np.int64)
        ctx = self._context_for_cells(ctx, res["chains"], res["chain_index"], lens, both_strands, int(p.band)) if C else ctx
        al = align_dev(lib, ctx, self.device, d_text, n, d["d_reads"], d["d_ridx"], d["Q"], both_strands, out["d_chains"],
                       out["d_cidx"], C, p, want_cigar)
        res.update(align_arrays(al, want_cigar))
        return res, _Aligned(lib=lib, ctx=ctx, d_text=d_text, n=n, d_reads=d["d_reads"], d_ridx=d["d_ridx"], Q=d["Q"], lens=lens,
                             d_cidx=out["d_cidx"], d_alns=al["d_alns"], C=C, al=al, align_params=p, keep=(d, out))

    def _context_for_cells(self, ctx, chains, chain_index, lens, both_strands, band):
        """the traceback store of an align call holds ALIGN_CELLS_PER_N cells per base of the context: ctx, or a context sized
        for these chains (numpy: the chain records, their index over the virtual reads, the read lengths)"""
        from .fm_align import ALIGN_CELLS_PER_N, ALIGN_MAX_BAND
        per_v = np.diff(chain_index.astype(np.int64))
        vlen = np.repeat(lens, 2) if both_strands else lens
        d0 = chains["tbeg"].astype(np.int64) - chains["rbeg"].astype(np.int64)
        d1 = chains["tend"].astype(np.int64) - chains["rend"].astype(np.int64)
        B = np.abs(d0 - d1) + 2 * band + 1
        cells = int((np.repeat(vlen, per_v) * np.where(B > ALIGN_MAX_BAND, 0, B)).sum())
        if cells > ALIGN_CELLS_PER_N * ctx.max_n:
            ctx = self._context(min(_lib.MAX_N, cells // ALIGN_CELLS_PER_N + (1 << 20)))
        return ctx

    # ---- the mappings of every read (kiss_hip_fmi_select_dev; no reference counterpart) ---------------------------------
    def map(self, reads, text, min_len=19, max_len=0, max_occ=500, both_strands=False, chain_params=None, align_params=None,
            bounds=None, want_cigar=True, want_md=False, **select_params):
        """Seeds, chains, alignments and the selection of every read's mappings (include/kiss_hip.h has the definition),
        with everything staying on the device between the four calls.  reads, text and the seed parameters as in align();
        chain_params / align_params: dicts of the parameters of chains() / align(); bounds: the starts of the R records of
        the text plus n (R + 1 ascending values, the first 0), None: one record; select_params: min_score (30), overlap
        (128, in 256ths), mapq_coef (120), mapq_max (60), max_hits (0: all).  Returns what align() returns plus hits
        (structured array: aln, flags, mapq, score, sub, n_sec, head, ref; flags 1 reverse, 2 secondary, 4 supplementary),
        hit_index (Q + 1: the hits of read q are hits[hit_index[q]:hit_index[q + 1]], the primary first) and select_report.
        want_md (it needs want_cigar): also md, md_index, md_counts and md_report -- the MD:Z string of every hit, in the order
        of hits (kiss_hip_fmi_md_dev, include/kiss_hip_md.h; kiss_amd.fm_md.md_strings() splits the bytes).
        Further keywords: sam (False; it needs want_cigar): also sam (bytes: the alignment lines of the batch, written from the buffers that are still on
        the device by kiss_hip_fmi_sam_dev, include/kiss_hip_sam.h; kiss_amd.sam_header() gives the lines in front of them),
        sam_line_index (lines + 1), sam_read_line (Q + 1: the first line of every read) and sam_report; with want_md the lines
        carry MD:Z:.  names: the QNAMEs, a list of str or bytes or the (raw, name_off, name_len) triple of parse_reads; None: the
        decimal read number.  qual: the quality bytes, a list with one entry per read or one array under the index of the reads;
        None prints '*'.  ref_names: the names of the R records, needed when bounds is given; without either RNAME is '*'.
        bam (False; it needs want_cigar, ref_names and bounds; names and qual as for sam, and both may be given): also bam (bytes: the
        BGZF blocks of the batch's BAM records, ready to append to a file behind the framed kiss_amd.bam_writer.bam_header(); written and
        framed on the device by kiss_hip_fmi_bam_dev and kiss_hip_bgzf_dev, include/kiss_hip_bam.h), bam_rec_index (records + 1, over
        the unframed records), bam_read_rec (Q + 1) and bam_report.
        bam_compress (False; it needs bam): the blocks are compressed on the device (DEFLATE, kiss_hip_bgzf_deflate_dev,
        include/kiss_hip_deflate.h); the result also has bam_block_index (blocks + 1, over bam) and bam_report the counts of the coding.
        bam_sort (False; it needs bam, and goes with bam_compress): the records of the batch are put into coordinate order on the
        device between the record call and the framing (kiss_hip_bam_sort_dev, include/kiss_hip_bam_sort.h): bam holds the sorted
        records and bam_rec_index is their CSR; the new bam_order (records, u32) says which record stands in every slot --
        bam_read_rec keeps counting the records as they were written, so record bam_read_rec[q] of read q is in the slot s with
        bam_order[s] == bam_read_rec[q] --, and bam_report gains unplaced and the times of the sort.  (A FILE is sorted as a whole
        by kiss_amd.bam_writer.write_bam(sort=True): sorted batches do not concatenate into a sorted file.)
        bam_markdup (False; it needs bam): True or dict(min_qual=15): the duplicate templates of the batch get FLAG 0x400 on the
        device between the record call and the sort or the framing (kiss_hip_bam_markdup_dev, include/kiss_hip_markdup.h, which has
        the definition); the new bam_dup (records, u8) says which records, numbered as they were written (as bam_read_rec counts
        them, with or without bam_sort), belong to one, and bam_markdup_report holds the counts.  (The duplicates of a FILE are
        marked by kiss_amd.bam_writer.write_bam(sort=True, markdup=True): they are a property of the file, not of a batch.)
        pileup (None; it needs want_cigar): True, a dict of lo, hi, counts and the pileup parameters min_mapq (0), skip_flags (2:
        secondary hits) and proper_only (0), or an (8, W) int32 device tensor to add to (the dict's counts: such a tensor, or an
        (8, W) u32 array): also pileup -- the eight planes of kiss_amd.fm_pileup.PLANES over the text positions [lo, hi), default
        the whole text, counted from the hits by kiss_hip_fmi_pileup_dev (include/kiss_hip_pileup.h) from the buffers that are
        still on the device; a u32 array, or the tensor that was given, now holding the sums -- and pileup_report."""
        from .fm_select import select_arrays, select_params as make_select_params
        so = self._sam_options(select_params, want_cigar, bounds)
        po = self._pileup_options(select_params, want_cigar)
        sp = make_select_params(**select_params)
        self._md_needs_ops(want_md, want_cigar)
        res, t = self._align_dev(reads, text, min_len, max_len, max_occ, both_strands, chain_params, want_cigar,
                                 align_params or {})
        ctx, sel = self._select(t, t.ctx, t.d_alns, t.d_cidx, t.C, both_strands, bounds, sp)
        res.update(select_arrays(sel))
        if want_md:
            res.update(self._md_of_hits(t, ctx, t.d_alns, t.d_cidx, t.C, t.al["d_cigar"], t.al["d_oidx"], both_strands, sel, so))
        if so:
            res.update(self._sam_lines(t, ctx, t.d_alns, t.C, t.al["d_cigar"], t.al["d_oidx"], sel, so))
        if po:
            res.update(self._pileup_counts(t, ctx, t.d_alns, t.d_cidx, t.al["d_cigar"], t.al["d_oidx"], both_strands, sel, po))
        return res

    @staticmethod
    def _md_needs_ops(want_md, want_cigar):
        if want_md and not want_cigar:
            raise ValueError("want_md needs the ops: want_cigar=True")

    def _select(self, t, ctx, d_alns, d_cidx, C, both_strands, bounds, sp):
        """the select stage over C alignments of the batch t -> the context it ran on (ctx, or one that sorts C alignments: a
        call sorts them in the context's LMS arrays) and select_dev's output.  (What select_arrays makes of it the caller
        merges into its result where it copies the rest: the rescue pass does so after its pair call.)"""
        from .fm_select import select_dev
        ctx = self._context_to_sort(ctx, C)
        return ctx, select_dev(t.lib, ctx, self.device, d_alns, d_cidx, t.d_ridx, t.Q, C, both_strands, bounds, sp)

    def _md_of_hits(self, t, ctx, d_alns, d_cidx, C, d_cigar, d_oidx, both_strands, sel, so=None):
        """map(want_md=True): the MD strings of the hits of a select call, from the buffers that are on the device (so: the SAM
        options, which keep the tensors for the lines)"""
        from .fm_md import md_arrays, md_dev
        out = md_dev(t.lib, ctx, self.device, t.d_text, t.n, t.d_reads, t.d_ridx, t.Q, both_strands, d_alns, d_cidx, C,
                     d_cigar, d_oidx, sel["d_hits"], int(sel["rep"].hits))
        if so:
            so["md"] = out
        return md_arrays(out)

    @staticmethod
    def _pileup_options(given, want_cigar):
        """map(pileup=...): takes pileup out of the keywords `given` -> None without it, else lo, hi, counts and the parameters,
        held against their limits before anything runs"""
        from .fm_pileup import WINDOW_KEYS, pileup_params
        what = given.pop("pileup", None)
        if what is None or what is False:
            return None
        if not want_cigar:
            raise ValueError("pileup needs the ops: want_cigar=True")
        opts = dict(what) if isinstance(what, dict) else ({} if what is True else {"counts": what})
        po = {k: opts.pop(k, None) for k in WINDOW_KEYS}
        pileup_params(**opts)
        po["params"] = opts
        return po

    def _pileup_counts(self, t, ctx, d_alns, d_cidx, d_cigar, d_oidx, both_strands, sel, po, out=None):
        """map(pileup=...): the counts of the hits of a select call (out: and the pairs of a pair call), from the buffers that are
        on the device"""
        from .fm_pileup import pileup_dev, planes_of, window
        torch = _torch()
        lo, hi = window(t.n, po["lo"] or 0, po["hi"])
        counts = po["counts"]
        on_device = isinstance(counts, torch.Tensor)
        if counts is not None and not on_device:
            host = np.ascontiguousarray(counts, dtype=np.uint32)
            if host.shape != (8, hi - lo):
                raise ValueError("the counts of a pileup have the shape (8, %d)" % (hi - lo))
            counts = torch.from_numpy(host.view(np.int32)).to(torch.device("cuda", self.device))
        got = pileup_dev(t.lib, ctx, self.device, t.d_text, t.n, t.d_reads, t.d_ridx, t.Q, both_strands, d_alns, d_cidx, d_cigar, d_oidx,
                         sel["d_hits"], int(sel["rep"].hits), out["d_pairs"] if out else None, int(out["rep"].P) if out else 0, lo, hi,
                         counts, **po["params"])
        return {"pileup": got["d_counts"] if on_device else planes_of(got["d_counts"]), "pileup_report": got["rep"].as_dict()}

    @staticmethod
    def _sam_options(given, want_cigar, bounds):
        """map(sam=..., bam=...): takes sam, bam, names, qual and ref_names out of the keywords `given` -> None without both, else the
        arguments of the lines, held against each other before anything runs"""
        sam, names, qual, ref_names = (given.pop(k, d) for k, d in (("sam", False), ("names", None), ("qual", None), ("ref_names", None)))
        bam = given.pop("bam", False)
        bam_compress = given.pop("bam_compress", False)
        bam_sort = given.pop("bam_sort", False)
        bam_unframed = given.pop("_bam_unframed", False)  # (write_bam(sort=True): the records stay on the device, unframed)
        bam_markdup = given.pop("bam_markdup", False)
        if bam_markdup and not bam:
            raise ValueError("bam_markdup belongs to bam=True")
        if bam_markdup:
            from .bam_writer import markdup_options
            bam_markdup = markdup_options(bam_markdup)
        if bam_compress and not bam:
            raise ValueError("bam_compress belongs to bam=True")
        if (bam_sort or bam_unframed) and not bam:
            raise ValueError("bam_sort belongs to bam=True")
        if not sam and not bam:
            if names is not None or qual is not None or ref_names is not None:
                raise ValueError("names, qual and ref_names belong to sam=True")
            return None
        if not want_cigar:
            raise ValueError("%s needs the ops: want_cigar=True" % ("sam" if sam else "bam"))
        if bam and (not ref_names or bounds is None):
            raise ValueError("bam needs the records: ref_names and bounds")
        from .fm_select import _bounds_array
        b = _bounds_array(bounds)
        R = len(ref_names) if ref_names is not None else 0
        if b is not None and R != b.size - 1:
            raise ValueError("ref_names has one name per record: bounds has R + 1 = %d entries" % b.size)
        if R > 1 and b is None:
            raise ValueError("ref_names with more than one name needs bounds")
        return {"names": names, "qual": qual, "ref_names": ref_names, "bounds": b, "md": None, "sam": bool(sam), "bam": bool(bam),
                "bam_compress": bool(bam_compress), "bam_sort": bool(bam_sort), "bam_unframed": bool(bam_unframed), "bam_markdup": bam_markdup or None}

    def _sam_lines(self, t, ctx, d_alns, C, d_cigar, d_oidx, sel, so, d_pairs=None, d_source=None, first_alns=0):
        """map(sam=True): the lines of the hits of a select call (and the pairs of a pair call), from the buffers that are on the
        device; names, qualities and record names go up beside them"""
        from .sam_writer import default_names, name_index, pack_names, sam_arrays, sam_lines_dev
        torch = _torch()
        dev = torch.device("cuda", self.device)
        Q, paired = t.Q, d_pairs is not None

        def up(a, as_type=None):  # (one element when it is empty: no NULL)
            a = np.ascontiguousarray(a)
            a = a if a.size else np.zeros(1, a.dtype)
            return torch.from_numpy(a.view(as_type) if as_type else a).to(dev)

        names = so["names"]
        if names is None:
            names = default_names(Q, paired)
        elif paired and not isinstance(names, tuple) and len(names) == Q // 2:
            names = [x for x in names for _ in (0, 1)]  # (one name per pair: both mates carry it)
        raw, noff, nlen = pack_names(names)
        if noff.size != Q or nlen.size != Q:
            raise ValueError("names has one entry per read (%d), or per pair" % Q)
        if Q and int((noff + nlen).max()) > raw.size:
            raise ValueError("a name span points past the name bytes")
        bases = int(t.lens.sum())
        qual = so["qual"]
        d_qual = None
        if qual is not None:
            if isinstance(qual, torch.Tensor):
                d_qual = qual.to(device=dev, dtype=torch.uint8).contiguous().reshape(-1)
                n_qual = int(d_qual.numel())
                d_qual = d_qual if n_qual else torch.zeros(1, dtype=torch.uint8, device=dev)
            else:
                if isinstance(qual, (list, tuple)):
                    parts = [np.frombuffer(x, np.uint8) if isinstance(x, (bytes, bytearray)) else np.ascontiguousarray(x, dtype=np.uint8).ravel()
                             for x in qual]
                    if [p.size for p in parts] != [int(x) for x in t.lens]:
                        raise ValueError("qual has one entry per read, as long as the read")
                    qual = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
                qual = np.ascontiguousarray(qual, dtype=np.uint8).ravel()
                n_qual, d_qual = qual.size, up(qual)
            if n_qual < bases:
                raise ValueError("qual covers %d bases, the reads have %d" % (n_qual, bases))
        b, ref_names = so["bounds"], so["ref_names"]
        R = len(ref_names) if ref_names is not None else 0
        if R and b is None:
            b = np.array([0, t.n], np.uint64)
        rn, rnidx = name_index(ref_names)
        md = so["md"]
        H = int(sel["rep"].hits)
        ctx = self._context_to_sort(ctx, Q + H + 1)
        arrays = dict(reads=t.d_reads, read_index=t.d_ridx, qual=d_qual, names=up(raw), name_off=up(noff, np.int64), name_len=up(nlen, np.int32),
                      alns=d_alns, cigar=d_cigar, cigar_index=d_oidx, hits=sel["d_hits"], hit_index=sel["d_hidx"], pairs=d_pairs, source=d_source,
                      md=md["d_md"] if md else None, md_index=md["d_midx"] if md else None, ref_names=up(rn) if R else None,
                      ref_name_index=up(rnidx, np.int64) if R else None, bounds=up(b, np.int64) if R else None)
        res = {}
        if so["sam"]:
            res.update(sam_arrays(sam_lines_dev(t.lib, ctx, self.device, Q, C, R, first_alns, **arrays)))
        if so["bam"]:  # (the records, then their blocks: both from the buffers on the device)
            from .bam_writer import bam_arrays, bam_marked, bam_records_dev, bam_sorted, bam_unframed
            out = bam_records_dev(t.lib, ctx, self.device, Q, C, R, first_alns, **arrays)
            if so["bam_markdup"]:  # (in place, in the order the records were written: before any sort)
                ctx = self._context_to_sort(ctx, int(out["rep"].records))
                out = bam_marked(t.lib, ctx, self.device, out, R, **so["bam_markdup"])
            if so["bam_unframed"]:
                res.update(bam_unframed(out))
            else:
                if so["bam_sort"]:
                    ctx = self._context_to_sort(ctx, int(out["rep"].records))
                    out = bam_sorted(t.lib, ctx, self.device, out, R)
                res.update(bam_arrays(t.lib, ctx, self.device, out, compress=so["bam_compress"]))
        return res

    # ---- the mappings of two mates paired (kiss_hip_fmi_pair_dev; no reference counterpart) -----------------------------
    def map_pairs(self, reads1, reads2, text, min_len=19, max_len=0, max_occ=500, chain_params=None, align_params=None,
                  select_params=None, bounds=None, want_cigar=True, rescue=None, want_md=False, insert=None, **pair_params):
        """map() for paired reads (forward-then-reverse libraries; include/kiss_hip.h has the definition): reads1[p] and
        reads2[p] are mate 1 and mate 2 of pair p, both as read from the sequencer.  They are interleaved into one batch
        (reads 2 p and 2 p + 1), which goes through seeds, chains, alignments and select on both strands and then through the
        pair call, everything staying on the device.  reads1 / reads2: equally many reads, each a list of uint8 arrays or
        (concatenated, index); select_params: a dict of the select parameters of map(); pair_params: ins_min (0), ins_max
        (1000), ins_mean (400), pen_coef (8, in 256ths), pen_max (20), mapq_coef (120), mapq_max (60).  Returns what map()
        returns for the interleaved batch plus pairs (structured array, one per pair: hit1, hit2 -- indices into hits, or
        0xFFFFFFFF --, flags, tlen, score, sub1, sub2, mapq1, mapq2, n_conc; flags 1 proper, 2 / 4 mate 1 / 2 mapped, 8 same
        record, 16 / 32 mate 1 / 2 promoted from a secondary) and pair_report.
        rescue: None, or True / a dict of the rescue parameters -- ins_min and ins_max (the pair parameters' unless given),
        max_anchors (4), min_anchor_score (0), max_width (960) --: the pairs that are not proper are planned into windows next
        to the hits of either mate (kiss_hip_fmi_rescue_dev), the windows aligned, their alignments merged behind the reads'
        own (kiss_hip_fmi_aln_merge_dev) and select and pair run again, everything staying on the device.  alignments,
        chain_index, cigar, cigar_index, hits, hit_index, pairs, select_report and pair_report are then those of the second
        pass over the merged set; `chains` stays the first pass's.  Added: aln_source (merged alignment a is alignment
        aln_source[a] of the first pass, whose chain has the same number, if that is below the first pass's count C_A, else
        it belongs to rescue chain aln_source[a] - C_A), first_pass (pairs, hits, hit_index, select_report, pair_report,
        alignments: C_A) and rescue (chains, chain_index, origin, report, align_report, merge_report, rescued: the pairs proper now and
        not before).
        want_md (it needs want_cigar): also md, md_index, md_counts and md_report, the MD:Z strings of `hits` as in map(); with
        rescue those of the second pass, from the merged alignments.
        insert: None, or "auto" / True / a dict of the insert parameters -- min_mapq (20), max_insert (10000), min_samples (25),
        out_mult (2), map_mult (3), sd_mult (4) --: the insert size is estimated from the first hits of the pairs between the
        select and the pair call (kiss_hip_fmi_insert_dev, include/kiss_hip_insert.h).  With enough samples ins_min, ins_max and
        ins_mean of the pair parameters are replaced by the estimate (every other pair parameter stays the caller's) and the
        rescue plan's ins_min / ins_max default to the estimated ones; otherwise the caller's or default values apply.  Added:
        insert (report, hist, applied, ins_min, ins_max, ins_mean: the three values used).  With rescue both passes use the
        same values: the estimate is taken once, from the first pass.
        Further keywords: sam (False; it needs want_cigar): also sam, sam_line_index, sam_read_line and sam_report as in map(), the paired lines of the
        interleaved batch; with rescue they come from the second pass and YR:i:1 follows aln_source.  names: one per pair (both
        mates carry it) or one per read of the interleaved batch; None: the decimal pair number.  qual: (qual1, qual2), each one
        entry per read of its file; ref_names as in map().  pileup as in map(), counted from the pairs (the chosen hit of every
        mate with the pair's MAPQ; proper_only: proper pairs alone); with rescue from the second pass's records and pairs."""
        from .fm_pair import pair_arrays, pair_dev, pair_params as make_pair_params
        from .fm_select import select_arrays, select_params as make_select_params
        so = self._sam_options(pair_params, want_cigar, bounds)
        po = self._pileup_options(pair_params, want_cigar)
        pp = make_pair_params(**pair_params)
        sp = make_select_params(**(select_params or {}))
        self._md_needs_ops(want_md, want_cigar)
        ip = None
        if insert is not None and insert is not False:
            from .fm_insert import insert_params as make_insert_params
            ip = make_insert_params(**({} if insert is True or insert == "auto" else dict(insert)))
        m1, m2 = read_list(reads1), read_list(reads2)
        if len(m1) != len(m2):
            raise ValueError("reads1 has %d reads, reads2 has %d: a pair has one of each" % (len(m1), len(m2)))
        batch = [r for pair in zip(m1, m2) for r in pair]
        if so and so["qual"] is not None:
            qual = so["qual"]
            if not isinstance(qual, (list, tuple)) or len(qual) != 2 or len(qual[0]) != len(m1) or len(qual[1]) != len(m2):
                raise ValueError("qual is (qual1, qual2), each with one entry per read of its file")
            so["qual"] = [x for pair in zip(qual[0], qual[1]) for x in pair]
        return self._map_pair_batch(batch, text, min_len, max_len, max_occ, chain_params, align_params, sp, bounds, want_cigar, rescue,
                                    want_md, ip, pp, so, po)

    def _map_pair_batch(self, batch, text, min_len, max_len, max_occ, chain_params, align_params, sp, bounds, want_cigar, rescue, want_md,
                        ip, pp, so=None, po=None):
        """map_pairs() behind its arguments: batch holds the mates interleaved (reads 2 p and 2 p + 1), in either form"""
        from .fm_pair import pair_arrays, pair_dev
        from .fm_select import select_arrays
        res, t = self._align_dev(batch, text, min_len, max_len, max_occ, True, chain_params, want_cigar, align_params or {})
        ctx, sel = self._select(t, t.ctx, t.d_alns, t.d_cidx, t.C, True, bounds, sp)
        res.update(select_arrays(sel))
        if ip is not None:
            pp = self._insert_estimate(res, t, ctx, sel, pp, ip)
        out = pair_dev(t.lib, ctx, self.device, sel["d_hits"], sel["d_hidx"], t.Q, t.d_alns, t.C, pp)
        res.update(pair_arrays(out))
        if rescue is None or rescue is False:
            if want_md:
                res.update(self._md_of_hits(t, ctx, t.d_alns, t.d_cidx, t.C, t.al["d_cigar"], t.al["d_oidx"], True, sel, so))
            if so:
                res.update(self._sam_lines(t, ctx, t.d_alns, t.C, t.al["d_cigar"], t.al["d_oidx"], sel, so, out["d_pairs"]))
            if po:
                res.update(self._pileup_counts(t, ctx, t.d_alns, t.d_cidx, t.al["d_cigar"], t.al["d_oidx"], True, sel, po, out))
            return res
        return self._rescue_pass(res, t, ctx, sel, out, sp, pp, bounds, want_cigar, {} if rescue is True else dict(rescue), want_md, so, po)

    def _insert_estimate(self, res, t, ctx, sel, pp, ip):
        """map_pairs(insert=...): the estimate from the hits of the first select call -> the pair parameters to use"""
        from .fm_insert import INSERT_OK, insert_arrays, insert_dev
        got = insert_arrays(insert_dev(t.lib, ctx, self.device, sel["d_hits"], sel["d_hidx"], t.Q, t.d_alns, t.C, ip))
        rep = got["report"]
        applied = bool(rep["flags"] & INSERT_OK)
        if applied:
            pp = _lib.PairParams(rep["ins_min"], rep["ins_max"], rep["ins_mean"], pp.pen_coef, pp.pen_max, pp.mapq_coef, pp.mapq_max)
        res["insert"] = dict(report=rep, hist=got["hist"], applied=applied, ins_min=int(pp.ins_min), ins_max=int(pp.ins_max),
                             ins_mean=int(pp.ins_mean))
        return pp

    def _rescue_pass(self, res, t, ctx, sel, out, sp, pp, bounds, want_cigar, rescue, want_md=False, so=None, po=None):
        """map_pairs(rescue=...): plan, the rescue align call, merge, and select and pair again (res: the first pass's result)"""
        from .fm_align import align_arrays, align_dev
        from .fm_pair import PAIR_PROPER, pair_arrays, pair_dev
        from .fm_rescue import merge_arrays, merge_dev, rescue_arrays, rescue_dev, rescue_params
        from .fm_select import select_arrays
        rescue.setdefault("ins_min", pp.ins_min)
        rescue.setdefault("ins_max", pp.ins_max)
        rp = rescue_params(**rescue)
        lib, Q, CA = t.lib, t.Q, t.C
        first = {k: res[k] for k in ("pairs", "hits", "hit_index", "select_report", "pair_report")}
        first["alignments"] = CA
        pl = rescue_dev(lib, ctx, self.device, out["d_pairs"], sel["d_hits"], sel["d_hidx"], Q, t.d_alns, CA, t.d_ridx, t.n,
                        bounds, rp, int(sel["rep"].hits))
        plan = rescue_arrays(pl)
        if pl["C"]:
            ctx = self._context_for_cells(ctx, plan["chains"], plan["chain_index"], t.lens, True, int(t.align_params.band))
        al2 = align_dev(lib, ctx, self.device, t.d_text, t.n, t.d_reads, t.d_ridx, Q, True, pl["d_chains"], pl["d_cidx"],
                        pl["C"], t.align_params, want_cigar)
        al1 = t.al
        a = {"d_alns": al1["d_alns"], "d_cidx": t.d_cidx, "C": CA, "d_cigar": al1["d_cigar"], "d_oidx": al1["d_oidx"],
             "ops": int(al1["rep"].cigar_ops)}
        b = {"d_alns": al2["d_alns"], "d_cidx": pl["d_cidx"], "C": pl["C"], "d_cigar": al2["d_cigar"], "d_oidx": al2["d_oidx"],
             "ops": int(al2["rep"].cigar_ops)}
        mg = merge_dev(lib, ctx, self.device, 2 * Q, a, b, want_cigar)
        C = mg["C"]
        ctx, sel2 = self._select(t, ctx, mg["d_alns"], mg["d_cidx"], C, True, bounds, sp)
        out2 = pair_dev(lib, ctx, self.device, sel2["d_hits"], sel2["d_hidx"], Q, mg["d_alns"], C, pp)
        res.update(merge_arrays(mg, want_cigar))
        res.update(select_arrays(sel2))
        res.update(pair_arrays(out2))
        if want_md:
            res.update(self._md_of_hits(t, ctx, mg["d_alns"], mg["d_cidx"], C, mg["d_cigar"], mg["d_oidx"], True, sel2, so))
        if so:
            res.update(self._sam_lines(t, ctx, mg["d_alns"], C, mg["d_cigar"], mg["d_oidx"], sel2, so, out2["d_pairs"], mg["d_source"], CA))
        if po:
            res.update(self._pileup_counts(t, ctx, mg["d_alns"], mg["d_cidx"], mg["d_cigar"], mg["d_oidx"], True, sel2, po, out2))
        proper1 = (first["pairs"]["flags"] & PAIR_PROPER) != 0
        proper2 = (res["pairs"]["flags"] & PAIR_PROPER) != 0
        plan.update(align_report=align_arrays(al2, False)["align_report"], merge_report=mg["rep"].as_dict(),
                    rescued=int(np.count_nonzero(proper2 & ~proper1)))
        res.update(first_pass=first, rescue=plan)
        return res

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
