"""numpy restatement of biovoltron FMIndex<SA_INTV, uint32_t, ...>{.LOOKUP_LEN} (reference
include/biovoltron/algo/align/exact_match/fm_index.hpp): build from (S, SA), the `.fmi` serialisation of both layouts,
get_range with stop_cnt and get_offsets in the reference's FIFO order.  A helper of the tests, not a conftest; it knows
nothing of the GPU code.

  occ(c, i)   = rows r < i, r != pri, with bwt[r] == c           (compute_occ, :166-182)
  lf(c, i)    = cnt[c] + occ(c, i)                               (:184-187)
  lookup_[K]  = beg of the backward search of rhash(K, L) from (0, N), no early stop; lookup_[4^L] = N  (:238-270)
  get_range   = lookup prologue, then compute_range with stop_upper = stop_cnt + 1 in u32 arithmetic   (:553-584, 224-235)
  get_offsets = sa_[beg, end) for SA_INTV = 1, else the breadth-first walk of depth < SA_INTV         (:453-501)
"""
import struct

import numpy as np

OCC1_INTV, OCC2_INTV, B_OCC_INTV = 256, 16, 64
U32 = 0xFFFFFFFF


class FmModel:
    def __init__(self, S, SA, sa_intv=4, lookup_len=0, with_lookup=True):
        S = np.asarray(S, dtype=np.uint8)
        SA = np.asarray(SA, dtype=np.int64)
        self.sa_intv, self.lookup_len = int(sa_intv), int(lookup_len)
        N = self.N = SA.size
        assert N == S.size + 1
        self.SA = SA
        self.pri = int(np.flatnonzero(SA == 0)[0])
        bwt = np.zeros(N, np.uint8)
        nz = SA != 0
        bwt[nz] = S[SA[nz] - 1] & 3
        self.bwt = bwt
        # R[c][i] = occ(c, i): the pri row ('$', stored as A) is never counted
        onehot = np.zeros((4, N), np.uint32)
        onehot[bwt[nz], np.flatnonzero(nz)] = 1
        self.R = np.zeros((4, N + 1), np.int64)
        np.cumsum(onehot, axis=1, out=self.R[:, 1:])
        tot = self.R[:, N]
        self.cnt = np.array([1, 1 + tot[0], 1 + tot[0] + tot[1], 1 + tot[0] + tot[1] + tot[2]], np.int64)
        # occ1 / occ2 (build_occ, :283-301): counts before each 256-row block / inside the block before each 16-row chunk
        rows1 = np.arange(N // OCC1_INTV + 1) * OCC1_INTV
        self.occ1 = self.R[:, rows1].T.astype(np.uint32)
        rows2 = np.arange(N // OCC2_INTV + 1) * OCC2_INTV
        self.occ2 = (self.R[:, rows2] - self.R[:, (rows2 // OCC1_INTV) * OCC1_INTV]).T.astype(np.uint8)
        # sa_ / b_ / b_occ_ (build_sa, :331-370)
        if self.sa_intv == 1:
            self.sa = SA.astype(np.uint32)
            self.b = self.b_occ = None
            self.brank = None
        else:
            b = (SA % self.sa_intv) == 0
            self.b = b
            self.brank = np.zeros(N + 1, np.int64)
            np.cumsum(b, out=self.brank[1:])
            self.b_occ = self.brank[np.arange(N // B_OCC_INTV + 1) * B_OCC_INTV].astype(np.uint32)
            self.sa = SA[b].astype(np.uint32)
        self.lookup = self.build_lookup() if with_lookup else None

    # ---- LF ----------------------------------------------------------------------------------------------------------
    def lf(self, c, i):
        return self.cnt[c] + self.R[c, i]

    def search_keys(self, keys, L):
        """(beg, end) of the backward search of rhash(K, L) from (0, N) for every K of `keys`, no early stop"""
        keys = np.asarray(keys, dtype=np.int64)
        beg = np.zeros(keys.size, np.int64)
        end = np.full(keys.size, self.N, np.int64)
        for j in range(L):  # the last character first: bits 2j of the key hold character L - 1 - j
            c = (keys >> (2 * j)) & 3
            beg = self.lf(c, beg)
            end = self.lf(c, end)
        return beg, end

    def build_lookup(self):
        L = self.lookup_len
        beg, _ = self.search_keys(np.arange(4 ** L), L)
        return np.concatenate([beg, [self.N]]).astype(np.uint32)

    # ---- serialisation (save, :591-615) --------------------------------------------------------------------------------
    def serialize(self):
        N = self.N
        out = [self.cnt.astype("<u4").tobytes(), struct.pack("<I", self.pri)]

        def vec(count, raw):
            out.append(struct.pack("<Q", count))
            out.append(raw)
        pad = np.zeros((-N) % 4, np.uint8)
        d = np.concatenate([self.bwt, pad]).reshape(-1, 4).astype(np.uint8)
        vec(N, (d[:, 0] | (d[:, 1] << 2) | (d[:, 2] << 4) | (d[:, 3] << 6)).astype(np.uint8).tobytes())
        vec(self.occ1.shape[0], self.occ1.astype("<u4").tobytes())
        vec(self.occ2.shape[0], self.occ2.tobytes())
        vec(self.sa.size, self.sa.astype("<u4").tobytes())
        vec(self.lookup.size, self.lookup.astype("<u4").tobytes())
        if self.sa_intv != 1:
            bits = np.concatenate([self.b, np.zeros((-N) % 64, bool)])
            vec(N, np.packbits(bits, bitorder="little").tobytes())
            vec(self.b_occ.size, self.b_occ.astype("<u4").tobytes())
        return b"".join(out)

    # ---- get_range (:553-584) -------------------------------------------------------------------------------------------
    def get_ranges(self, patterns, stop_cnt=0):
        """-> beg, end, offs for a (Q, Lp) batch, literally the reference's get_range(seed, stop_cnt) per row"""
        P = np.asarray(patterns, dtype=np.int64) & 3
        Q, Lp = P.shape
        L = self.lookup_len
        beg = np.zeros(Q, np.int64)
        end = np.full(Q, self.N, np.int64)
        length = np.full(Q, Lp, np.int64)
        if Lp >= L:
            key = np.zeros(Q, np.int64)
            for i in range(Lp - L, Lp):
                key = (key << 2) | P[:, i]
            beg = self.lookup[key].astype(np.int64)
            end = self.lookup[key + 1].astype(np.int64)
            length[:] = Lp - L
        stop_upper = (int(stop_cnt) + 1) & U32
        early = (end == beg) | (length == 0)  # get_range(seed, beg, end, stop_cnt): offset 0
        active = ~early
        for pos in range(Lp - 1, -1, -1):
            here = active & (length == pos + 1)
            active &= ~(here & ((end - beg) < stop_upper))  # compute_range stops for good once the range is too small
            step = here & active
            c = P[:, pos]
            beg = np.where(step, self.lf(c, beg), beg)
            end = np.where(step, self.lf(c, end), end)
            length = np.where(step, length - 1, length)
        offs = np.where(early, 0, length)
        return beg.astype(np.uint32), end.astype(np.uint32), offs.astype(np.uint32)

    # ---- get_offsets (:453-501) -----------------------------------------------------------------------------------------
    def get_offsets(self, beg, end):
        beg, end = int(beg), int(end)
        if self.sa_intv == 1:
            return self.sa[beg:end].astype(np.uint64)
        want = end - beg
        out = []
        got = 0
        cb = np.array([beg], np.int64)
        ce = np.array([end], np.int64)
        for dep in range(self.sa_intv):  # FIFO order = level order; one level at a time
            if cb.size == 0 or got >= want:
                break
            ob, oe = self.brank[cb], self.brank[ce]
            cnt = oe - ob
            excl = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            proc = got + excl < want  # the reference tests offsets.size() < end - beg before every range
            np_ = int(proc.sum())      # (a prefix)
            total = int(cnt[:np_].sum())
            if total:  # sa_[ob[k], oe[k]) of the processed ranges, one after the other
                idx = np.repeat(ob[:np_] - excl[:np_], cnt[:np_]) + np.arange(total)
                out.append(self.sa[idx].astype(np.uint64) + dep)
            got += total
            if np_ < cb.size or dep + 1 == self.sa_intv:
                break
            pb, pe = cb[:np_], ce[:np_]
            single = pb + 1 == pe
            nb = np.empty((np_, 4), np.int64)
            ne = np.empty((np_, 4), np.int64)
            for c in range(4):
                nb[:, c] = self.lf(c, pb)
                ne[:, c] = self.lf(c, pe)
            sb = self.lf(self.bwt[pb].astype(np.int64), pb)  # one row: its own character (pri: the stored A)
            nb[single] = -1
            ne[single] = -1
            nb[single, 0] = sb[single]
            ne[single, 0] = sb[single] + 1
            keep = nb != ne
            cb, ce = nb[keep], ne[keep]
        return np.concatenate(out) if out else np.zeros(0, np.uint64)

    def query_batch(self, patterns, stop_cnt=0, want_offsets=True):
        beg, end, offs = self.get_ranges(patterns, stop_cnt)
        res = {"beg": beg, "end": end, "offs": offs}
        per = [self.get_offsets(b, e) for b, e in zip(beg.tolist(), end.tolist())]
        counts = np.array([p.size for p in per], np.uint64)
        res["total_hits"] = int(counts.sum())
        res["checksum"] = int(sum(int(p.sum()) for p in per))
        if want_offsets:
            res["offsets_index"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
            res["offsets"] = (np.concatenate(per) if per else np.zeros(0, np.uint64)).astype(np.uint32)
        return res


# ---- the layout of both instantiations ----------------------------------------------------------------------------------
def sections(buf, sa_intv):
    """-> dict name -> (offset of the payload, count, payload bytes), N; b_ and b_occ_ only when sa_intv != 1"""
    names = [("bwt", None), ("occ1", 16), ("occ2", 4), ("sa", 4), ("lookup", 4)]
    if sa_intv != 1:
        names += [("b", None), ("b_occ", 4)]
    off, out, N = 20, {}, None
    for name, esz in names:
        (count,) = struct.unpack_from("<Q", buf, off)
        off += 8
        if name == "bwt":
            N = count
            nbytes = (count + 3) // 4
        elif name == "b":
            nbytes = ((count + 63) // 64) * 8
        else:
            nbytes = count * esz
        out[name] = (off, count, nbytes)
        off += nbytes
    assert off == len(buf), "trailing or missing bytes in .fmi"
    return out, N


def expected_counts(N, sa_intv, lookup_len):
    c = {"bwt": N, "occ1": N // OCC1_INTV + 1, "occ2": N // OCC2_INTV + 1, "sa": (N + sa_intv - 1) // sa_intv,
         "lookup": 4 ** lookup_len + 1}
    if sa_intv != 1:
        c.update(b=N, b_occ=N // B_OCC_INTV + 1)
    return c


def lookup_of(buf, sa_intv):
    sec, _ = sections(buf, sa_intv)
    off, count, _ = sec["lookup"]
    return np.frombuffer(buf, dtype="<u4", count=count, offset=off)
