"""The BGZF framing on the device (kiss_hip_bgzf_dev / _host; include/kiss_hip_bam.h) against the framing model of
tests/bam_model.py, byte for byte, and against Python's gzip: the sizes around one block, block lengths from one byte to the
largest, payloads whose CRC lanes start at every byte phase, data and out at every address, the end-of-file block, the capacity
rule, the caller's arrays on both sides of 2^31 and across a multiple of 2^32."""
import ctypes
import gzip

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bam_model as B
from tests.test_fm_sam_gpu import GUARD, PAD, guarded, guards_intact

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 65279, 65280, 65281, 65505, 200000)
BLOCKS = (1, 7, 65280, 65505)
RANDOM = np.random.default_rng(77).integers(0, 256, (4 << 20) + 1, dtype=np.uint8)


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 20, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


def frame_dev(gpu, data, bb, eof, data_shift=0, out_shift=0, cap=None, out_view=None, data_view=None):
    """data (uint8 array) framed on the device -> (status, report, the bytes of out, out untouched?, guards intact?)"""
    import torch
    lib, ctx, dev = gpu
    vp = ctypes.c_void_p
    n = int(data.size)
    total = B.out_bytes(n, bb, eof)
    cap = total if cap is None else cap
    din_whole, din = guarded(dev, max(n, 1), data_shift)
    if data_view is not None:
        din = data_view[:max(n, 1)]
    if n:
        din[:n].copy_(torch.from_numpy(data.copy()))
    out_whole, out = out_view if out_view is not None else guarded(dev, max(cap, 1), out_shift)
    assert data_view is not None or din.data_ptr() % 16 == (PAD + data_shift) % 16
    rep = _lib.BgzfReport()
    rc = lib.kiss_hip_bgzf_dev(ctx._ctx, vp(din.data_ptr()) if n else None, n, bb, int(eof), vp(out.data_ptr()), cap, ctypes.byref(rep), None)
    got = out.cpu().numpy()
    return rc, rep, got[:total].tobytes(), bool(np.all(got == GUARD)), guards_intact(out_whole, out) and bool(np.all(got[total:] == GUARD))


def check(gpu, data, bb, eof, what, **where):
    rc, rep, got, _, intact = frame_dev(gpu, data, bb, eof, **where)
    want = B.frame(data.tobytes(), bb, eof)
    assert rc == 0, what
    assert (int(rep.blocks), int(rep.out_bytes)) == (-(-data.size // (bb or 65280)), len(want)), what
    if got != want:
        k = next(i for i in range(len(want)) if got[i] != want[i])
        block, at = divmod(k, (bb or 65280) + 31)
        raise AssertionError("%s: out differs at byte %d, byte %d of block %d: got %r, want %r" % (what, k, at, block, got[k - 4:k + 8], want[k - 4:k + 8]))
    assert intact, what
    return got


@pytest.mark.parametrize("eof", [False, True])
@pytest.mark.parametrize("bb", BLOCKS)
def test_the_sizes_around_a_block(gpu, bb, eof):
    for n in SIZES:
        got = check(gpu, RANDOM[:n], bb, eof, "n %d, block_bytes %d" % (n, bb))
        if got:
            assert gzip.decompress(got) == RANDOM[:n].tobytes(), (n, bb)
        assert got.endswith(B.BGZF_EOF) == eof or not n


def test_four_mebibytes_and_a_byte_and_the_default_block(gpu):
    got = check(gpu, RANDOM, 0, True, "4 MiB + 1")
    assert gzip.decompress(got) == RANDOM.tobytes() and got == B.frame(RANDOM.tobytes(), 65280, True)


@pytest.mark.parametrize("fill", ["zeros", "ff", "random"])
def test_payloads(gpu, fill):
    n = 3 * 65280 + 1021
    data = {"zeros": np.zeros(n, np.uint8), "ff": np.full(n, 255, np.uint8), "random": RANDOM[1:n + 1]}[fill]
    for bb in (0, 1021, 1020 * 64, 255 * 256 + 1):
        check(gpu, data, bb, False, "%s, block_bytes %d" % (fill, bb))


def test_data_at_every_address_mod_16_and_out_at_odd_addresses(gpu):
    for shift in range(16):
        for n in (1, 2, 3, 4, 5, 65280 + 9):
            check(gpu, RANDOM[shift:shift + n], 0, shift % 2 == 0, "data at %d mod 16, n %d" % (shift, n), data_shift=shift, out_shift=(3 * shift + 1) % 16)
    for out_shift in (1, 3, 5, 7):
        check(gpu, RANDOM[:70000], 4099, True, "out at %d" % out_shift, out_shift=out_shift)


def test_eof_alone_and_nothing_at_all(gpu):
    assert check(gpu, RANDOM[:0], 0, True, "eof alone") == B.BGZF_EOF
    rc, rep, got, untouched, intact = frame_dev(gpu, RANDOM[:0], 0, False, cap=8)
    assert rc == 0 and (int(rep.blocks), int(rep.out_bytes)) == (0, 0) and untouched and intact


def test_capacity_one_short_and_block_bytes_out_of_range(gpu):
    for n, bb, eof in ((1000, 0, True), (65281, 0, False), (10, 3, True), (0, 0, True)):
        total = B.out_bytes(n, bb, eof)
        rc, rep, _, untouched, intact = frame_dev(gpu, RANDOM[:n], bb, eof, cap=total - 1)
        assert rc == _lib.KISS_HIP_E_INVALID and (int(rep.blocks), int(rep.out_bytes)) == (-(-n // (bb or 65280)), total), (n, bb)
        assert untouched and intact
    for bb in (65506, 1 << 20, 0xFFFFFFFF):
        rc, rep, _, untouched, intact = frame_dev(gpu, RANDOM[:100], 7, False, cap=4096)
        assert rc == 0
        lib, ctx, dev = gpu
        whole, out = guarded(dev, 4096)
        _, din = guarded(dev, 100)
        rep = _lib.BgzfReport()
        rc = lib.kiss_hip_bgzf_dev(ctx._ctx, ctypes.c_void_p(din.data_ptr()), 100, bb, 0, ctypes.c_void_p(out.data_ptr()), 4096, ctypes.byref(rep), None)
        assert rc == _lib.KISS_HIP_E_INVALID and np.all(out.cpu().numpy() == GUARD) and guards_intact(whole, out), bb


def test_the_host_entry_and_the_python_wrappers(gpu):
    import torch
    import kiss_amd.bam_writer as W
    lib, ctx, dev = gpu
    x = RANDOM[:150001].tobytes()
    assert W.bgzf(x) == B.frame(x) and W.bgzf(x, 4099, True) == B.frame(x, 4099, True) and W.bgzf(b"", eof=True) == B.BGZF_EOF and W.bgzf(b"") == b""
    got, rep = W.bgzf(np.frombuffer(x, np.uint8), 65505, want_report=True)
    assert got == B.frame(x, 65505) and rep["blocks"] == 3 and rep["out_bytes"] == len(got)
    d_out, rep = W.bgzf_dev(lib, ctx, 0, torch.from_numpy(RANDOM[:150001].copy()).to(dev), 150001, eof=True)
    assert d_out.cpu().numpy().tobytes() == B.frame(x, eof=True) and int(rep.blocks) == 3


def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    import torch
    lib, ctx, dev = gpu
    data = RANDOM[5:5 + 2 * 65280 + 77]
    total = B.out_bytes(data.size, 0, True)
    G = 1 << 32
    arena = torch.empty(G + (64 << 20), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    to_carry = (-base) % G
    high = (to_carry + (1 << 31) + 4096) % G
    places = {"high half": high if high >= PAD else high + G, "low half": to_carry + 4096,
              "across a multiple of 2^32": to_carry - 1024 if to_carry >= 1024 + PAD else to_carry + G - 1024}
    for what, off in places.items():
        lo = (base + off) & (G - 1)
        assert {"high half": lo >= 1 << 31, "low half": lo < 1 << 31, "across a multiple of 2^32": lo == G - 1024}[what]
        assert off >= PAD and off + total + PAD <= arena.numel()
        whole = arena[off - PAD:off + total + PAD]
        whole.fill_(GUARD)
        check(gpu, data, 0, True, "out at " + what, out_view=(whole, whole[PAD:PAD + total]))
        check(gpu, data, 0, True, "data at " + what, data_view=arena[off + 1:])
    del arena
