"""BGZF blocks compressed on the device (kiss_hip_bgzf_deflate_dev / _host; include/kiss_hip_deflate.h) against the
encoder restated in tests/deflate_model.py -- out byte for byte, block_index and every count of the report -- and against Python's
gzip, which is the check that does not share the model's reading of the format: the payloads of tests/deflate_cases.py at block
lengths from one byte to the largest, every length up to 300 for four fills, 500 random payloads with planted repeats, the sizes
around a block, a mebibyte of mixed data with all three codings side by side,
data and out at every address, both capacity rules, the guards behind out_bytes, the caller's stream, the host entry and the
Python wrappers, the caller's arrays on both sides of 2^31 and across a multiple of 2^32."""
import ctypes
import gzip

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from tests import bam_model as B
from tests import deflate_cases as C
from tests import deflate_model as D
from tests.test_fm_sam_gpu import GUARD, PAD, guarded, guards_intact

pytestmark = pytest.mark.gpu

COUNTS = ("blocks", "out_bytes", "stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches", "match_bytes")
SHORT_BLOCKS = (1, 7, 255, 256, 257, 4099, 65280, 65505)
SHORT = C.short_cases()
LONG = C.long_cases()
MODEL = {}


def model(data, bb):
    """the model's (bytes without the end-of-file block, block_index, counts), computed once per (data, block_bytes)"""
    key = (data, bb)
    if key not in MODEL:
        MODEL[key] = D.frame_report(data, bb, False)
    return MODEL[key]


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 20, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


def deflate_dev(gpu, data, bb, eof, data_shift=0, out_shift=0, cap=None, icap=None, out_view=None, data_view=None, stream=None, index=True):
    """data (bytes) compressed on the device -> (status, report, all of out, block_index, guards intact?)"""
    import torch
    lib, ctx, dev = gpu
    vp = ctypes.c_void_p
    n = len(data)
    bound = B.out_bytes(n, bb, eof)
    blocks = -(-n // (bb or 65280))
    cap = bound if cap is None else cap
    icap = blocks + 1 if icap is None else icap
    din_whole, din = guarded(dev, max(n, 1), data_shift)
    if data_view is not None:
        din = data_view[:max(n, 1)]
    if n:
        din[:n].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    out_whole, out = out_view if out_view is not None else guarded(dev, max(cap, 1), out_shift)
    assert data_view is not None or din.data_ptr() % 16 == (PAD + data_shift) % 16
    d_index = torch.full((max(icap, 1) + 2,), -1, dtype=torch.int64, device=dev)
    rep = _lib.BgzfDeflateReport()
    rc = lib.kiss_hip_bgzf_deflate_dev(ctx._ctx, vp(din.data_ptr()) if n else None, n, bb, int(eof), vp(out.data_ptr()), cap,
                                       vp(d_index.data_ptr()) if index else None, icap, ctypes.byref(rep), vp(stream) if stream else None)
    return rc, rep, out.cpu().numpy(), d_index.cpu().numpy(), guards_intact(out_whole, out) and (data_view is not None or guards_intact(din_whole, din))


def check(gpu, data, bb, eof, what, **where):
    rc, rep, got, index, intact = deflate_dev(gpu, data, bb, eof, **where)
    blocks, want_index, want_rep = model(data, bb)
    want = blocks + (B.BGZF_EOF if eof else b"")
    assert rc == 0, what
    got_rep = {k: int(getattr(rep, k)) for k in COUNTS}
    assert got_rep == dict(want_rep, out_bytes=len(want)), what
    out = got[:len(want)].tobytes()
    if out != want:
        k = next(i for i in range(len(want)) if out[i] != want[i])
        b = max(i for i, at in enumerate(want_index) if at <= k)
        raise AssertionError("%s: out differs at byte %d, byte %d of block %d: got %r, want %r" % (what, k, k - want_index[b], b, out[k - 4:k + 8], want[k - 4:k + 8]))
    if where.get("index", True):
        assert index[:len(want_index)].tolist() == want_index and np.all(index[len(want_index):] == -1), what
    assert intact and np.all(got[len(want):] == GUARD), what   # nothing behind out_bytes, up to the worst-case capacity
    if want:
        assert gzip.decompress(out) == data, what
    return out


@pytest.mark.parametrize("bb", SHORT_BLOCKS)
def test_short_payloads_at_every_block_length(gpu, bb):
    for name, P in SHORT.items():
        if bb < 255 and len(P) > 2000:   # (thousands of tiny blocks show nothing that hundreds do not)
            P = P[:1500]
        check(gpu, P, bb, bb % 2 == 1, "%s, block_bytes %d" % (name, bb))


@pytest.mark.parametrize("name", sorted(LONG))
def test_long_payloads(gpu, name):
    for bb in (0, 65505):
        check(gpu, LONG[name], bb, bb == 0, "%s, block_bytes %d" % (name, bb))


@pytest.mark.parametrize("fill", ["zeros", "ff", "random", "text"])
def test_every_length_up_to_300(gpu, fill):
    """a call per length, the block as long as the payload, for the four fills of the CPU list"""
    src = {"zeros": bytes(300), "ff": b"\xff" * 300, "random": C.RANDOM[7:307], "text": C.text()[5000:5300]}[fill]
    for n in range(1, 301):
        check(gpu, src[:n], 0, n % 2 == 1, "%s, %d bytes" % (fill, n))


@pytest.mark.parametrize("part", range(5))
def test_random_payloads_with_planted_repeats(gpu, part):
    """the 500 payloads of the CPU list (the same generator and seed), a call each: small alphabets, dense short matches, colliding
    hashes, copies that overlap themselves"""
    rng = np.random.default_rng(4)
    payloads = [C.planted(rng) for _ in range(500)]
    kinds = set()
    for k in range(100 * part, 100 * part + 100):
        check(gpu, payloads[k], 0, k % 2 == 0, "payload %d" % k)
        kinds |= {c for c in ("stored_blocks", "fixed_blocks", "dynamic_blocks") if model(payloads[k], 0)[2][c]}
    assert len(kinds) == 3


@pytest.mark.parametrize("eof", [False, True])
def test_the_sizes_around_a_block(gpu, eof):
    for n in (0, 1, 3, 4, 5, 65279, 65280, 65281, 200000):
        for fill, src in (("random", C.RANDOM), ("period 256", C.period(256, 200000))):
            got = check(gpu, src[:n], 0, eof, "%s, n %d" % (fill, n))
            assert got.endswith(B.BGZF_EOF) == eof or not n
    assert check(gpu, b"", 0, True, "eof alone") == B.BGZF_EOF
    # random bytes do not shrink: the stored blocks of kiss_hip_bgzf_dev, byte for byte
    assert check(gpu, C.RANDOM[:200000], 0, True, "random") == B.frame(C.RANDOM[:200000], 0, True)


def mixed_mebibyte():
    """random stretches, runs and text, whose lengths do not go with the block length: blocks that stay stored, blocks of a few
    long matches (the fixed codes win: a dynamic header costs more than it saves) and blocks of text (dynamic) in turn"""
    text, parts, k = C.text(), [], 0
    while sum(map(len, parts)) < 1 << 20:
        parts += [C.RANDOM[k * 997:k * 997 + 9000 + k], bytes([k % 251]) * (7000 + 3 * k), text[(k * 1013) % 30000:][:12000 + 7 * k]]
        k += 1
    return b"".join(parts)[:1 << 20]


def test_a_mebibyte_with_stored_fixed_and_dynamic_blocks_side_by_side(gpu):
    data = mixed_mebibyte()
    assert len(data) == 1 << 20
    check(gpu, data, 4099, True, "a mebibyte")
    rep = model(data, 4099)[2]
    assert rep["stored_blocks"] > 20 and rep["fixed_blocks"] > 20 and rep["dynamic_blocks"] > 20, rep


def test_data_at_every_address_mod_16_and_out_at_odd_addresses(gpu):
    text = C.text()
    for shift in range(16):
        for n in (1, 2, 3, 4, 5, 2000 + shift):
            check(gpu, text[shift:shift + n], 0, shift % 2 == 0, "data at %d mod 16, n %d" % (shift, n), data_shift=shift, out_shift=(3 * shift + 1) % 16)
    for out_shift in (1, 3, 5, 7):
        check(gpu, LONG["records with qualities"][:70000], 4099, True, "out at %d" % out_shift, out_shift=out_shift)
        check(gpu, C.RANDOM[:70000], 4099, True, "stored, out at %d" % out_shift, out_shift=out_shift, data_shift=out_shift + 1)


def test_both_capacities_one_short_leave_out_untouched(gpu):
    for n, bb, eof in ((1000, 0, True), (65281, 0, False), (10, 3, True), (0, 0, True)):
        bound, blocks = B.out_bytes(n, bb, eof), -(-n // (bb or 65280))
        rc, rep, got, index, intact = deflate_dev(gpu, C.text()[:n], bb, eof, cap=bound - 1)
        assert rc == _lib.KISS_HIP_E_INVALID and (int(rep.blocks), int(rep.out_bytes)) == (blocks, bound), (n, bb)
        assert np.all(got == GUARD) and np.all(index == -1) and intact
        rc, rep, got, index, intact = deflate_dev(gpu, C.text()[:n], bb, eof, icap=blocks)
        assert rc == _lib.KISS_HIP_E_INVALID and np.all(got == GUARD) and np.all(index == -1) and intact, (n, bb)
        check(gpu, C.text()[:n], bb, eof, "no index", index=False)
    for bb in (65506, 1 << 20, 0xFFFFFFFF):
        rc, rep, got, index, intact = deflate_dev(gpu, C.text()[:100], 7, False)
        assert rc == 0
        lib, ctx, dev = gpu
        whole, out = guarded(dev, 4096)
        _, din = guarded(dev, 100)
        rep = _lib.BgzfDeflateReport()
        rc = lib.kiss_hip_bgzf_deflate_dev(ctx._ctx, ctypes.c_void_p(din.data_ptr()), 100, bb, 0, ctypes.c_void_p(out.data_ptr()), 4096, None, 0,
                                           ctypes.byref(rep), None)
        assert rc == _lib.KISS_HIP_E_INVALID and np.all(out.cpu().numpy() == GUARD) and guards_intact(whole, out), bb


def test_the_callers_stream_with_a_decoy_on_another(gpu):
    import torch
    lib, ctx, dev = gpu
    data, decoy = LONG["records without qualities"][:100000], LONG["text"]
    want = model(data, 0)[0]
    mine, other = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    ctx2 = kiss_amd.Context(max_n=1 << 20, device=0)
    try:
        d_in = torch.zeros(len(data), dtype=torch.uint8, device=dev)
        staged = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(dev)
        d_decoy = torch.from_numpy(np.frombuffer(decoy, np.uint8).copy()).to(dev)
        busy = torch.zeros(64 << 20, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(mine):   # the data arrives on the caller's stream, behind work that takes a while
            for _ in range(8):
                busy.add_(1)
            d_in.copy_(staged)
        import kiss_amd.bam_writer as W
        with torch.cuda.stream(other):
            d_other, _, _ = W.bgzf_deflate_dev(lib, ctx2, 0, d_decoy, len(decoy))
        d_out, d_index, rep = W.bgzf_deflate_dev(lib, ctx, 0, d_in, len(data), stream=mine.cuda_stream)
        assert d_out.cpu().numpy().tobytes() == want and d_index.cpu().numpy().tolist() == model(data, 0)[1]
        assert d_other.cpu().numpy().tobytes() == model(decoy, 0)[0]
    finally:
        ctx2.close()


def test_the_host_entry_and_the_python_wrappers(gpu):
    import torch
    import kiss_amd.bam_writer as W
    lib, ctx, dev = gpu
    x = LONG["records with qualities"][:150001]
    blocks, index, rep = model(x, 0)
    assert W.bgzf_deflate(x) == blocks and W.bgzf_deflate(x, eof=True) == blocks + B.BGZF_EOF
    got, got_index, got_rep = W.bgzf_deflate(np.frombuffer(x, np.uint8), 4099, True, want_report=True, want_index=True)
    want, want_index, want_rep = model(x, 4099)
    assert got == want + B.BGZF_EOF and got_index.tolist() == want_index
    assert {k: got_rep[k] for k in COUNTS} == dict(want_rep, out_bytes=len(want) + 28)
    d_out, d_index, drep = W.bgzf_deflate_dev(lib, ctx, 0, torch.from_numpy(np.frombuffer(x, np.uint8).copy()).to(dev), len(x), eof=True)
    assert d_out.cpu().numpy().tobytes() == blocks + B.BGZF_EOF and d_index.cpu().numpy().tolist() == index and int(drep.blocks) == len(index) - 1 == 2
    assert gzip.decompress(got) == x


def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    import torch
    lib, ctx, dev = gpu
    data = LONG["records with qualities"][5:5 + 65280 + 77] + C.RANDOM[:65280]
    bound = B.out_bytes(len(data), 0, True)
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
        assert off >= PAD and off + bound + PAD <= arena.numel()
        whole = arena[off - PAD:off + bound + PAD]
        whole.fill_(GUARD)
        check(gpu, data, 0, True, "out at " + what, out_view=(whole, whole[PAD:PAD + bound]))
        check(gpu, data, 0, True, "data at " + what, data_view=arena[off + 1:])
    del arena
