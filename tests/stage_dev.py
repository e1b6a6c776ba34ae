"""Raw ctypes calls of the stage entry points (include/kiss_hip.h) on torch device tensors, for tests/test_stage_*_gpu.py:
guarded caller buffers, the ctx's own views as numpy arrays."""
import ctypes

import numpy as np

E_INVALID, E_DEEP = -1, -8
VIEW_LOCAL_KEYS, VIEW_LOCAL_POS, VIEW_PART_KEYS, VIEW_PART_POS, VIEW_SORTED, VIEW_SORTED_CTX = range(6)
GUARD = 64                      # entries behind what a call may write
GUARD64, GUARD32 = 0x5A5A5A5A5A5A5A5A, 0x6B6B6B6B


class Stage:
    def __init__(self, ctx):
        import torch
        import kiss_amd
        self.torch, self.ctx, self.lib = torch, ctx, getattr(ctx, "_lib", None) or kiss_amd.load()
        self.dev = torch.device("cuda", 0)
        self.texts = {}

    # ---- data ------------------------------------------------------------------------------------------------------------
    def upload(self, S):
        """the text on the device (once per text)"""
        if id(S) not in self.texts:
            self.texts[id(S)] = (S, self.torch.from_numpy(np.array(S)).to(self.dev))
        return self.texts[id(S)][1]

    def to_dev(self, a, room=0):
        """a u32 / u64 array on the device, with `room` guard entries behind it -> (the tensor, its first len(a) entries)"""
        a = np.ascontiguousarray(a)
        signed, guard = {4: (np.int32, GUARD32), 8: (np.int64, GUARD64)}[a.dtype.itemsize]
        whole = np.concatenate([a, np.full(room, guard, dtype=a.dtype)])
        t = self.torch.from_numpy(whole.view(signed)).to(self.dev)
        return t, t[:a.size]

    def guarded(self, count, bytes_each):
        """`count` entries to be written by a call, GUARD entries behind them, all holding the guard value"""
        dt, guard = {4: (self.torch.int32, GUARD32), 8: (self.torch.int64, GUARD64)}[bytes_each]
        return self.torch.full((count + GUARD,), guard, dtype=dt, device=self.dev)

    @staticmethod
    def host(t, count, dtype, what="output"):
        """the first `count` entries of a guarded tensor; the guard behind them must be intact"""
        a = t.cpu().numpy().view(dtype)
        guard = GUARD32 if a.dtype.itemsize == 4 else GUARD64
        assert np.all(a[count:] == guard), what + ": written behind its end"
        return a[:count].copy()

    @staticmethod
    def ptr(t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None

    def sync(self):
        self.torch.cuda.synchronize(self.dev)

    # ---- calls -------------------------------------------------------------------------------------------------------------
    def classify(self, S, k, lo, hi, n=None, counts=True):
        """-> (rc, the 13 counters)"""
        d_S = self.upload(S)
        self.sync()
        c = (ctypes.c_uint64 * 13)()
        rc = self.lib.kiss_hip_stage_classify(self.ctx._ctx, ctypes.c_void_p(d_S.data_ptr()), len(S) if n is None else n,
                                              int(k) & 0xFFFFFFFF, int(lo), int(hi), ctypes.byref(c) if counts else None, None)
        return rc, [int(x) for x in c]

    def sizes(self):
        m, mf = ctypes.c_uint64(), ctypes.c_uint64()
        assert self.lib.kiss_hip_stage_local_lms(self.ctx._ctx, None, None, ctypes.byref(m), ctypes.byref(mf)) == 0
        return int(m.value), int(mf.value)

    def copy_list(self):
        """the copy form of stage_local_lms into guarded caller tensors -> (keys, pos) on the host"""
        m, _ = self.sizes()
        keys, pos = self.guarded(m, 8), self.guarded(m, 4)
        self.sync()
        m2, mf2 = ctypes.c_uint64(), ctypes.c_uint64()
        rc = self.lib.kiss_hip_stage_local_lms(self.ctx._ctx, self.ptr(keys), self.ptr(pos), ctypes.byref(m2), ctypes.byref(mf2))
        assert rc == 0 and m2.value == m
        return self.host(keys, m, np.uint64, "copied keys"), self.host(pos, m, np.uint32, "copied positions")

    def view_tensor(self, which, count):
        """the first `count` entries of one of the ctx's work arrays, zero-copy (asked for anew: a regrowth moves them)"""
        from kiss_amd.multi_gpu import _DevArray
        p, cap = ctypes.c_void_p(), ctypes.c_uint64()
        assert self.lib.kiss_hip_stage_view(self.ctx._ctx, which, ctypes.byref(p), ctypes.byref(cap)) == 0
        assert count <= cap.value
        wide = which in (VIEW_LOCAL_KEYS, VIEW_PART_KEYS)
        if count == 0:
            return self.torch.empty(0, dtype=self.torch.int64 if wide else self.torch.int32, device=self.dev)
        return self.torch.as_tensor(_DevArray(p.value, count, "<i8" if wide else "<i4"), device=self.dev)

    def view(self, which, count):
        wide = which in (VIEW_LOCAL_KEYS, VIEW_PART_KEYS)
        return self.view_tensor(which, count).cpu().numpy().view(np.uint64 if wide else np.uint32).copy()

    def capacity(self):
        p, cap = ctypes.c_void_p(), ctypes.c_uint64()
        assert self.lib.kiss_hip_stage_view(self.ctx._ctx, VIEW_LOCAL_POS, ctypes.byref(p), ctypes.byref(cap)) == 0
        return int(cap.value)

    def sort(self, keys, pos, count, n, k, out, words):
        """stage_sort on device tensors (None = NULL) -> rc"""
        self.sync()
        return self.lib.kiss_hip_stage_sort(self.ctx._ctx, self.ptr(keys), self.ptr(pos), int(count), int(n), int(k) & 0xFFFFFFFF,
                                            self.ptr(out), self.ptr(words), None)

    def induce(self, n, k, far, words, near, counts12):
        """stage_induce on device tensors -> (rc, SA on the host); nothing may be written behind the SA"""
        sa = self.guarded(n + 1, 4)
        c = (ctypes.c_uint64 * 12)(*[int(x) for x in counts12])
        self.sync()
        rc = self.lib.kiss_hip_stage_induce(self.ctx._ctx, int(n), int(k) & 0xFFFFFFFF, self.ptr(far), self.ptr(words),
                                            int(far.numel()), self.ptr(near), int(near.numel()), ctypes.byref(c), self.ptr(sa), None)
        return rc, (self.host(sa, n + 1, np.uint32, "SA") if rc == 0 else None)
