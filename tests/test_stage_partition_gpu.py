"""The stage partition and the stage key histogram (kiss_amd/csrc/stages.hip) through their public entries, on torch
device tensors, against numpy.

kiss_hip_stage_partition is the one shipped caller of the radix sort's key_lo_bit = 64 form: no key pass, one pass over
the group ids (the sharded sort runs it with 1 to 3 groups only, tests/test_multi_gpu.py).  The group of a key is the
number of splitters <= its first `bits` bits, and the partition is stable.  kiss_hip_stage_key_hist counts those first
bits: in LDS up to 14 bits, with global atomics above."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 16384
E_INVALID = -1
MAX_N = 1_000_000  # m_cap = 324 096


@pytest.fixture(scope="module")
def env():
    import torch
    import kiss_amd
    ctx = kiss_amd.Context(max_n=MAX_N, device=0)
    yield ctx, kiss_amd.load(), torch, torch.device("cuda", 0)
    ctx.close()


def to_dev(torch, dev, a):
    signed = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}[a.dtype]
    return torch.from_numpy(a.view(signed).copy()).to(dev)


def to_host(t, dtype):
    return t.cpu().numpy().view(dtype)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def make_keys(n, bits, seed):
    """keys whose first `bits` bits take about forty values (so that a splitter can sit on one), the rest random"""
    rng = np.random.default_rng([n, bits, seed])
    bins = np.unique(rng.integers(0, 1 << bits, 40, dtype=np.uint64))
    top = bins[rng.integers(0, bins.size, n)]
    low = rng.integers(0, 1 << 63, n, dtype=np.uint64) & np.uint64((1 << (64 - bits)) - 1)
    keys = (top << np.uint64(64 - bits)) | low
    pos = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(99)).astype(np.uint32)
    return keys, pos, bins


def make_splitters(style, groups, bits, bins):
    """groups - 1 ascending splitters in units of the first `bits` key bits"""
    if groups == 1:
        return np.zeros(0, dtype=np.uint32)
    spread = lambda count: np.linspace(0, bins.size - 1, count + 2).astype(np.int64)[1:-1]
    if style == "between":  # none of them a value that occurs
        sp = [int(v) + 1 for v in bins[spread(groups - 1)]]
        for i in range(len(sp)):
            while sp[i] in bins:
                sp[i] += 1
        sp = np.minimum(np.array(sp, dtype=np.uint64), (1 << bits) - 1)
    elif style == "on_value":  # every splitter IS an occurring value: it belongs to the group it opens (<=)
        sp = bins[spread(groups - 1)]
    else:  # neighbouring splitters equal in pairs: the groups between them stay empty
        assert style == "equal" and groups > 2
        sp = np.repeat(bins[spread(groups // 2)], 2)[:groups - 1]
    return np.sort(sp).astype(np.uint32)


PARTITION_CASES = [(groups, style, n, bits)
                   for groups in (1, 2, 3, 64) for style in ("between", "on_value", "equal")
                   for n, bits in ((0, 16), (1, 16), (1000, 16), (TILE + 1, 16), (3 * TILE + 4097, 16), (TILE + 1, 7), (2 * TILE, 24))
                   if not (groups == 1 and style != "between") and not (groups == 2 and style == "equal")]


@pytest.mark.parametrize("groups,style,n,bits", PARTITION_CASES)
def test_stage_partition_is_a_stable_partition_by_group(env, groups, style, n, bits):
    ctx, lib, torch, dev = env
    keys, pos, bins = make_keys(n, bits, groups)
    sp = make_splitters(style, groups, bits, bins)
    assert sp.size == groups - 1 and np.all(sp[1:] >= sp[:-1])
    top = (keys >> np.uint64(64 - bits)).astype(np.int64)
    group = (top[:, None] >= sp.astype(np.int64)[None, :]).sum(1)
    order = np.argsort(group, kind="stable")
    if n > 1000 and groups > 1:  # the cases are what they claim
        assert np.unique(group).size > 1 and not np.array_equal(order, np.arange(n))
        if style == "on_value":
            assert np.isin(sp, bins).all()
        if style == "equal" and groups > 2:
            assert np.unique(sp).size < sp.size and np.unique(group).size < groups
    d_keys, d_pos = to_dev(torch, dev, keys), to_dev(torch, dev, pos)
    d_ko = torch.full((n,), -7, dtype=torch.int64, device=dev)
    d_po = torch.full((n,), -7, dtype=torch.int32, device=dev)
    c_sp = (ctypes.c_uint32 * max(1, groups - 1))(*[int(x) for x in sp])
    torch.cuda.synchronize(dev)
    rc = lib.kiss_hip_stage_partition(ctx._ctx, ptr(d_keys), ptr(d_pos), n, bits, c_sp, groups, ptr(d_ko), ptr(d_po), None)
    assert rc == 0, rc
    assert np.array_equal(to_host(d_po, np.uint32), pos[order])
    assert np.array_equal(to_host(d_ko, np.uint64), keys[order])
    assert np.array_equal(to_host(d_keys, np.uint64), keys) and np.array_equal(to_host(d_pos, np.uint32), pos)  # (inputs intact)


def test_stage_partition_argument_checks(env):
    ctx, lib, torch, dev = env
    n = 100
    keys, pos, _ = make_keys(n, 16, 0)
    d_keys, d_pos = to_dev(torch, dev, keys), to_dev(torch, dev, pos)
    d_ko, d_po = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    sp = (ctypes.c_uint32 * 63)(*range(1000, 1063))
    torch.cuda.synchronize(dev)

    def call(handle=ctx._ctx, k=d_keys, p=d_pos, count=n, bits=16, splitters=sp, groups=2, ko=d_ko, po=d_po):
        return lib.kiss_hip_stage_partition(handle, ptr(k), ptr(p), count, bits, splitters, groups, ptr(ko), ptr(po), None)

    assert call() == 0
    assert call(handle=None) == E_INVALID
    assert call(groups=0) == E_INVALID and call(groups=65) == E_INVALID and call(groups=64) == 0
    assert call(bits=0) == E_INVALID and call(bits=25) == E_INVALID and call(bits=1) == 0 and call(bits=24) == 0
    assert call(splitters=None) == E_INVALID and call(splitters=None, groups=1) == 0
    for missing in ("k", "p", "ko", "po"):
        assert call(**{missing: None}) == E_INVALID
        assert call(**{missing: None}, count=0) == 0  # nothing to read or write
    cap, view = ctypes.c_uint64(), ctypes.c_void_p()
    assert lib.kiss_hip_stage_view(ctx._ctx, 1, ctypes.byref(view), ctypes.byref(cap)) == 0
    assert call(count=cap.value + 1) == E_INVALID
    # in place: only where nothing moves (one group)
    assert call(ko=d_keys) == E_INVALID and call(po=d_pos) == E_INVALID
    assert call(ko=d_keys, po=d_pos, groups=1) == 0
    assert np.array_equal(to_host(d_keys, np.uint64), keys) and np.array_equal(to_host(d_pos, np.uint32), pos)


@pytest.mark.parametrize("bits", [14, 16])  # the LDS kernel / the global-atomic kernel
@pytest.mark.parametrize("n", [0, 100, 200_000])  # nothing, less than one workgroup, many with one hot bin
def test_stage_key_hist_counts_the_first_bits(env, bits, n):
    ctx, lib, torch, dev = env
    rng = np.random.default_rng([bits, n])
    keys = rng.integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1) | rng.integers(0, 2, n, dtype=np.uint64)
    hot = np.uint64(0x2B67 >> (16 - bits))
    if n > 1000:  # a poly-A like bin: 60 % of the keys, in runs (every lane of a wave on one counter)
        where = (np.arange(n) // 512) % 5 < 3
        keys[where] = (hot << np.uint64(64 - bits)) | (keys[where] >> np.uint64(bits))
    want = np.bincount((keys >> np.uint64(64 - bits)).astype(np.int64), minlength=1 << bits)
    assert want.size == 1 << bits and (n <= 1000 or want[int(hot)] > n // 2)
    d_keys = to_dev(torch, dev, keys)
    d_hist = torch.full((1 << bits,), 0x0123456789ABCDEF, dtype=torch.int64, device=dev)  # (the entry clears it)
    torch.cuda.synchronize(dev)
    rc = lib.kiss_hip_stage_key_hist(ctx._ctx, ptr(d_keys), n, bits, ptr(d_hist), None)
    assert rc == 0, rc
    assert np.array_equal(to_host(d_hist, np.uint64), want.astype(np.uint64))


def test_stage_key_hist_argument_checks(env):
    ctx, lib, torch, dev = env
    keys = np.arange(10, dtype=np.uint64) << np.uint64(50)
    d_keys = to_dev(torch, dev, keys)
    d_hist = torch.zeros(1 << 14, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, ptr(d_keys), 10, 14, ptr(d_hist), None) == 0
    assert lib.kiss_hip_stage_key_hist(None, ptr(d_keys), 10, 14, ptr(d_hist), None) == E_INVALID
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, ptr(d_keys), 10, 14, None, None) == E_INVALID
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, ptr(d_keys), 10, 0, ptr(d_hist), None) == E_INVALID
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, ptr(d_keys), 10, 25, ptr(d_hist), None) == E_INVALID
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, None, 10, 14, ptr(d_hist), None) == E_INVALID
    assert lib.kiss_hip_stage_key_hist(ctx._ctx, None, 0, 14, ptr(d_hist), None) == 0
    assert int(d_hist.sum().item()) == 0
