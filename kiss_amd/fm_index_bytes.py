"""FM-index over a byte text (values 0..255): build, `.fmi8` serialisation, batched search + locate over ragged patterns.

The counterpart of kiss_amd.fm_index.FMIndex for the general alphabet: built from the EXACT suffix array of the text
(kiss_hip_ctx_suffix_sort_u8_dev), served by the kiss_hip_fmi8_* entry points (include/kiss_hip.h; layout: DESIGN.md 4.7).
A hit of a pattern P is a position p with text[p : p + len(P)] == P; overlapping hits all count, positions come back in
ascending order per pattern.  No result depends on sa_intv.

All arithmetic runs in libkiss_hip.so through its C ABI; torch only owns the device buffers.  There is no CPU path.
"""
import ctypes
import struct

import numpy as np

from . import _lib
from .sorter import Context, _check

SA_INTV = 4
MAX_SA_INTV = 32  # KISS_HIP_FMI_MAX_SA_INTV
MAGIC = b"KISSFMI8"
FORMAT_VERSION = 1


def _torch():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("kiss_amd.FMIndexBytes needs a HIP device (no CPU fallback)")
    return torch


def _as_u8(data):
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8)


def sizes(n, sa_intv, sigma):
    """entries of every array of the index of a text of n bytes with sigma distinct values (kiss_hip_fmi8_sizes_for)"""
    z = _lib.Fmi8Sizes()
    _check(_lib.load().kiss_hip_fmi8_sizes_for(int(n), int(sa_intv), int(sigma), ctypes.byref(z)), "kiss_hip_fmi8_sizes_for")
    return z.as_dict()


# (array of the file, numpy dtype on disk, torch dtype name that holds it, key of sizes())
_ARRAYS = (("C", "<u4", "int32", None), ("map", "u1", "uint8", None), ("bwt", "u1", "uint8", "bwt_bytes"),
           ("occ1", "<u4", "int32", "occ1_entries"), ("occ2", "<u2", "int16", "occ2_entries"),
           ("sa", "<u4", "int32", "sa_entries"), ("b", "<u8", "int64", "b_words"), ("b_occ", "<u4", "int32", "b_occ_entries"))


class FMIndexBytes:
    def __init__(self, device=0, sa_intv=SA_INTV, hooks=None):
        """hooks is for the tests and the measuring tools only: True serves this index from libkiss_hip_hooks.so."""
        if not 1 <= int(sa_intv) <= MAX_SA_INTV:
            raise ValueError("sa_intv must be in 1..%d, got %d" % (MAX_SA_INTV, sa_intv))
        self.device = int(device)
        self.sa_intv = int(sa_intv)
        self._hooks = hooks
        self.N = 0
        self.pri = 0
        self.sigma = 0
        self.C = self.map = self.bwt = self.occ1 = self.occ2 = self.sa = self.b = self.b_occ = None  # device tensors
        self._ctx = None

    def _context(self, max_n):
        if self._ctx is None or self._ctx.max_n < max_n:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = Context(max_n=max(max_n, 1 << 20), device=self.device, hooks=self._hooks)
        return self._ctx

    def _sizes(self):
        z = sizes(self.N - 1, self.sa_intv, self.sigma)
        z["C"], z["map"] = 257, 256
        return z

    def _alloc(self, N, sigma):
        torch = _torch()
        dev = torch.device("cuda", self.device)
        self.N, self.sigma = int(N), int(sigma)
        z = self._sizes()
        for name, _, tdt, key in _ARRAYS:
            count = z[key or name]
            if name in ("b", "b_occ") and self.sa_intv == 1:
                setattr(self, name, None)
            else:  # (never an empty tensor: its data_ptr is NULL)
                setattr(self, name, torch.zeros(max(count, 1) + (1 if name == "b" else 0), dtype=getattr(torch, tdt), device=dev))

    # ---- build ---------------------------------------------------------------------------------------------------
    def build(self, text, sa=None):
        """text: bytes, a numpy uint8 array or a uint8 tensor of this device.  sa: the EXACT suffix array (n + 1 entries,
        sa[0] = n; numpy or a device tensor of 32-bit entries); None sorts the text on the device first."""
        torch = _torch()
        dev = torch.device("cuda", self.device)
        if isinstance(text, torch.Tensor):
            d_S = text.to(dev).contiguous()
        else:
            d_S = torch.from_numpy(np.array(_as_u8(text))).to(dev)
        n = int(d_S.numel())
        ctx = self._context(n)
        lib = _lib.load(self._hooks)
        vp = ctypes.c_void_p
        ptr = lambda t: vp(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        if sa is None:
            d_SA = torch.empty(n + 1, dtype=torch.int32, device=dev)
            _check(lib.kiss_hip_ctx_suffix_sort_u8_dev(ctx._ctx, ptr(d_S), n, ptr(d_SA), None),
                   "kiss_hip_ctx_suffix_sort_u8_dev", ctx._ctx)
        elif isinstance(sa, torch.Tensor):
            d_SA = sa.to(dev).contiguous()
        else:
            d_SA = torch.from_numpy(np.ascontiguousarray(sa, dtype=np.uint32).view(np.int32)).to(dev)
        if d_SA.numel() != n + 1 or d_SA.element_size() != 4:
            raise ValueError("sa must hold n + 1 32-bit entries")
        sigma, pri = ctypes.c_uint32(), ctypes.c_uint32()
        # the census first: the arrays are sized by the number of distinct byte values
        _check(lib.kiss_hip_fmi8_build_dev(ctx._ctx, ptr(d_S), n, None, self.sa_intv, 0, None, None, None, None, None, None,
                                           None, None, ctypes.byref(sigma), ctypes.byref(pri), None),
               "kiss_hip_fmi8_build_dev", ctx._ctx)
        self._alloc(n + 1, sigma.value)
        _check(lib.kiss_hip_fmi8_build_dev(ctx._ctx, ptr(d_S), n, ptr(d_SA), self.sa_intv, self.sigma, ptr(self.C),
                                           ptr(self.map), ptr(self.bwt), ptr(self.occ1), ptr(self.occ2), ptr(self.sa),
                                           ptr(self.b), ptr(self.b_occ), ctypes.byref(sigma), ctypes.byref(pri), None),
               "kiss_hip_fmi8_build_dev", ctx._ctx)
        self.pri = int(pri.value)
        return self

    # ---- FILE.fmi8 ----------------------------------------------------------------------------------
    # magic "KISSFMI8", u32 version, u32 sa_intv, u64 N, u32 pri, u32 sigma, then C, map, bwt, occ1, occ2, sa, b, b_occ, each
    # as a u64 count of entries + little-endian entries (b / b_occ with count 0 when sa_intv == 1)
    def to_bytes(self):
        z = self._sizes()
        out = [MAGIC, struct.pack("<IIQII", FORMAT_VERSION, self.sa_intv, self.N, self.pri, self.sigma)]
        for name, dt, _, key in _ARRAYS:
            t = getattr(self, name)
            count = z[key or name] if t is not None else 0
            out.append(struct.pack("<Q", count))
            if count:
                a = t[:count].cpu().numpy()
                out.append(a.view(np.dtype(dt).newbyteorder("=")).astype(dt).tobytes())
        return b"".join(out)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @classmethod
    def from_bytes(cls, buf, device=0, hooks=None):
        torch = _torch()
        mv = memoryview(buf)
        head = len(MAGIC) + struct.calcsize("<IIQII")
        if len(mv) >= len(MAGIC) and bytes(mv[:len(MAGIC)]) != MAGIC:
            raise ValueError("not a .fmi8 file (bad magic)")
        if len(mv) < head:
            raise ValueError("truncated .fmi8")
        version, sa_intv, N, pri, sigma = struct.unpack_from("<IIQII", mv, len(MAGIC))
        if version != FORMAT_VERSION:
            raise ValueError(".fmi8 format version %d, this build reads %d" % (version, FORMAT_VERSION))
        if not 1 <= sa_intv <= MAX_SA_INTV or N == 0 or N > _lib.MAX_N + 1 or sigma > 256 or pri >= N:
            raise ValueError("bad .fmi8 header")
        self = cls(device, sa_intv=sa_intv, hooks=hooks)
        self.N, self.sigma, self.pri = int(N), int(sigma), int(pri)
        z = self._sizes()
        off, raws = head, {}
        for name, dt, _, key in _ARRAYS:
            if off + 8 > len(mv):
                raise ValueError("truncated .fmi8")
            count = struct.unpack_from("<Q", mv, off)[0]
            off += 8
            want = 0 if (name in ("b", "b_occ") and sa_intv == 1) else z[key or name]
            if count != want:
                raise ValueError("%s of the .fmi8 has %d entries, the header needs %d" % (name, count, want))
            nbytes = count * np.dtype(dt).itemsize
            if off + nbytes > len(mv):
                raise ValueError("truncated .fmi8")
            raws[name] = np.frombuffer(mv[off:off + nbytes], dtype=dt)
            off += nbytes
        if off != len(mv):
            raise ValueError("trailing bytes in .fmi8")
        self._alloc(N, sigma)
        for name, dt, tdt, _ in _ARRAYS:
            t = getattr(self, name)
            if t is None or not raws[name].size:
                continue
            a = raws[name].astype(np.dtype(dt).newbyteorder("="))
            t[:a.size].copy_(torch.from_numpy(a.view(getattr(np, tdt))).to(t.device))
        return self

    @classmethod
    def load(cls, path, device=0, hooks=None):
        with open(path, "rb") as f:
            return cls.from_bytes(f.read(), device, hooks)

    # ---- queries ---------------------------------------------------------------------------------------------------
    def _view(self):
        v = _lib.Fmi8View()
        v.n_sa, v.pri, v.sa_intv, v.sigma = self.N, self.pri, self.sa_intv, self.sigma
        for name, _, _, _ in _ARRAYS:
            t = getattr(self, name)
            setattr(v, name, t.data_ptr() if t is not None else None)
        return v

    @staticmethod
    def _ragged(patterns):
        """-> (concatenated bytes as uint8 array, index as uint64 array of Q + 1)"""
        if isinstance(patterns, tuple):
            concat, index = patterns
            return _as_u8(concat), np.ascontiguousarray(index, dtype=np.uint64)
        lens = np.fromiter((len(p) for p in patterns), dtype=np.uint64, count=len(patterns))
        index = np.zeros(len(patterns) + 1, np.uint64)
        np.cumsum(lens, out=index[1:])
        return np.frombuffer(b"".join(bytes(p) for p in patterns), dtype=np.uint8), index

    def query_batch(self, patterns, want_positions=True):
        """patterns: a list of bytes, or (concat, index) with index = Q + 1 u64, the exclusive prefix of the lengths.
        Returns dict(beg, end, counts, total_hits, checksum, report) and, with want_positions, positions / index in CSR
        layout (index: Q + 1 u64), ascending position inside a pattern.  A batch with more hits than one call sorts is
        cut into parts; `report` sums the parts (`calls` of them)."""
        if self.bwt is None:
            raise ValueError("no index: build or load one first")
        torch = _torch()
        dev = torch.device("cuda", self.device)
        concat, pidx = self._ragged(patterns)
        Q = int(pidx.size) - 1
        if Q < 0:
            raise ValueError("index must hold Q + 1 entries")
        if Q and (int(pidx[0]) != 0 or np.any(pidx[1:] <= pidx[:-1]) or int(pidx[-1]) != concat.size):
            raise ValueError("patterns of length 0, or an index that is not the exclusive prefix of the lengths")
        lib = _lib.load(self._hooks)
        view = self._view()
        vp = ctypes.c_void_p
        d_pat = torch.from_numpy(np.array(concat)).to(dev) if concat.size else torch.zeros(1, dtype=torch.uint8, device=dev)
        d_pidx = torch.from_numpy(pidx.view(np.int64).copy()).to(dev)
        beg = torch.zeros(max(Q, 1), dtype=torch.int32, device=dev)
        end = torch.zeros(max(Q, 1), dtype=torch.int32, device=dev)
        acc = {"hits": 0, "lf_pairs": 0, "walk_failures": 0, "checksum": 0, "ms_total": 0.0, "ms_search": 0.0, "ms_locate": 0.0,
               "ms_sort": 0.0, "calls": 0, "ms_counts": 0.0}
        pos_parts = []

        def call(lo, hi, positions, index, cap):
            """patterns [lo, hi) -> (status, report)"""
            rep = _lib.Fmi8Report()
            tot, chk = ctypes.c_uint64(), ctypes.c_uint64()
            rc = lib.kiss_hip_fmi8_query_dev(self._ctx._ctx, ctypes.byref(view), vp(d_pat.data_ptr()), vp(d_pidx.data_ptr() + 8 * lo),
                                             hi - lo, vp(beg.data_ptr() + 4 * lo), vp(end.data_ptr() + 4 * lo), ctypes.byref(tot),
                                             ctypes.byref(chk), positions, index, cap, ctypes.byref(rep), None)
            return rc, rep

        def add(rep):
            for k in acc:
                if k not in ("calls", "ms_counts"):
                    acc[k] += getattr(rep, k)
            acc["calls"] += 1

        def locate(lo, hi, total):
            positions = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
            index = torch.empty(hi - lo + 1, dtype=torch.int64, device=dev)
            rc, rep = call(lo, hi, vp(positions.data_ptr()), vp(index.data_ptr()), total)
            if rc == _lib.KISS_HIP_E_UNSUPPORTED:
                return rc
            if rc == _lib.KISS_HIP_E_INVALID and rep.walk_failures:
                raise _lib.KissHipError(rc, "kiss_hip_fmi8_query_dev", "%d rows reached no sampled row: the index was not built "
                                        "from an exact suffix array" % rep.walk_failures)
            _check(rc, "kiss_hip_fmi8_query_dev", self._ctx._ctx)
            add(rep)
            pos_parts.append(positions[:total].cpu().numpy().view(np.uint32))
            return rc

        if Q:
            self._context(max(self.N, 4 * Q))
            rc, rep = call(0, Q, None, None, 0)  # the ranges of the whole batch: they size the output and say where to cut
            _check(rc, "kiss_hip_fmi8_query_dev", self._ctx._ctx)
            if not want_positions:
                add(rep)
            else:
                acc["ms_counts"] = float(rep.ms_total)
        h_beg = beg[:Q].cpu().numpy().view(np.uint32)
        h_end = end[:Q].cpu().numpy().view(np.uint32)
        counts = (h_end - h_beg).astype(np.uint64)
        ends = np.cumsum(counts.astype(np.int64))
        if Q and want_positions:
            cap = int(0.32 * self._ctx.max_n)
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
                _check(locate(lo, hi, total), "kiss_hip_fmi8_query_dev", self._ctx._ctx)
        rep = dict(acc)
        rep["Q"] = Q
        res = {"beg": h_beg, "end": h_end, "counts": counts, "total_hits": int(counts.sum()), "checksum": int(acc["checksum"]),
               "report": rep}
        if want_positions:
            res["positions"] = np.concatenate(pos_parts) if pos_parts else np.zeros(0, np.uint32)
            index = np.zeros(Q + 1, np.uint64)
            index[1:] = ends.astype(np.uint64)
            res["index"] = index
        return res

    def count(self, pattern):
        """occurrences of one pattern"""
        return int(self.query_batch([bytes(pattern)], want_positions=False)["counts"][0])

    def locate(self, pattern):
        """positions of one pattern, ascending (numpy uint32)"""
        return self.query_batch([bytes(pattern)])["positions"]

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
