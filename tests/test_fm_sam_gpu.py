"""The SAM lines written on the device (kiss_hip_fmi_sam_dev / _host; include/kiss_hip_sam.h) against their definition,
tests/fm_sam_model.py: every byte of sam, line_index, read_line and every field of the report but the times.  The batches are
made by the model's make_batch; outputs lie between guard bytes; bad reads, the size-then-fill protocol, odd addresses, the
caller's stream, the host entry, and arrays placed on both sides of 2^31 and across a multiple of 2^32."""
import ctypes

import numpy as np
import pytest

import kiss_amd
from kiss_amd import _lib
from kiss_amd.sam_writer import name_index, pack_names, sam_input
from tests import fm_sam_model as M

pytestmark = pytest.mark.gpu

GUARD, PAD = 0xA5, 64
REPORT = ("lines", "sam_bytes", "unmapped_lines", "longest", "bad", "first_bad")
BYTE_ARRAYS = ("reads", "qual", "names", "md", "ref_names")
WORD_ARRAYS = ("name_len", "alns", "cigar", "hits", "pairs", "source")


def rng_of(seed):
    return np.random.default_rng(seed)


def host_arrays(b):
    """the model's batch -> name -> numpy array in the library's layout (None stays None), and Q, C, R, first_alns"""
    raw, noff, nlen = pack_names(b["names"])
    rn, rnidx = name_index(b["ref_names"])
    R = len(b["ref_names"])
    u32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, np.int64).astype(np.uint32))  # noqa: E731
    u64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint64)  # noqa: E731
    arrs = {"reads": b["reads"], "read_index": u64(b["read_index"]), "qual": b["qual"], "names": raw, "name_off": noff, "name_len": nlen,
            "alns": u32(b["alns"]), "cigar": u32(b["cigar"]), "cigar_index": u64(b["cigar_index"]), "hits": u32(b["hits"]),
            "hit_index": u64(b["hit_index"]), "pairs": u32(b["pairs"]), "source": u32(b["source"]), "md": b["md"], "md_index": u64(b["md_index"]),
            "ref_names": rn if R else None, "ref_name_index": rnidx if R else None, "bounds": u64(b["bounds"]) if R else None}
    return arrs, (len(b["read_index"]) - 1, len(b["alns"]), R, int(b["first_alns"]))


def guarded(dev, nbytes, shift=0):
    """nbytes on the device between PAD guard bytes, `shift` bytes off the allocation's alignment -> (the whole tensor, the
    view of the nbytes)"""
    import torch
    t = torch.full((nbytes + 2 * PAD + shift,), GUARD, dtype=torch.uint8, device=dev)
    return t, t[PAD + shift:PAD + shift + nbytes]


def guards_intact(whole, view):
    w = whole.cpu().numpy()
    lo = view.data_ptr() - whole.data_ptr()
    return bool(np.all(w[:lo] == GUARD) and np.all(w[lo + view.numel():] == GUARD))


def put(dev, arrs, odd=False, place=None):
    """the arrays on the device -> name -> uint8 view (None stays None).  odd: byte arrays at an odd address, u32 arrays and
    records at 4 mod 8.  place: name -> a uint8 view of an arena to put that array into.  An empty array is one element."""
    import torch
    out, keep = {}, []
    for name, a in arrs.items():
        if a is None:
            out[name] = None
            continue
        raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        raw = raw if raw.size else np.zeros(8, np.uint8)
        if place and name in place:
            v = place[name][:raw.size]
        else:
            shift = 0 if not odd else (1 if name in BYTE_ARRAYS else (4 if name in WORD_ARRAYS else 0))
            whole, v = guarded(dev, raw.size, 8 + shift)  # (PAD + 8 keeps the 8-byte alignment of the index arrays)
            keep.append(whole)
        v.copy_(torch.from_numpy(raw.copy()))
        out[name] = v
        if odd and name in BYTE_ARRAYS + WORD_ARRAYS:
            assert v.data_ptr() % 8 == (1 if name in BYTE_ARRAYS else 4), name
    out["_keep"] = keep
    return out


class Outputs:
    def __init__(self, dev, sam_cap, line_cap, Q, odd=False, sam_view=None, want_lines=True):
        self.sam_whole, self.sam = guarded(dev, max(sam_cap, 1), 1 if odd else 0)
        if sam_view is not None:
            self.sam_whole, self.sam = sam_view
        self.li_whole, self.li = guarded(dev, 8 * (line_cap + 1), 8)
        self.rl_whole, self.rl = guarded(dev, 8 * (Q + 1), 8)
        self.sam_cap, self.line_cap, self.want_lines = sam_cap, line_cap, want_lines

    def untouched(self):
        return bool(np.all(self.sam.cpu().numpy() == GUARD) and np.all(self.li.cpu().numpy() == GUARD))

    def intact(self):
        return guards_intact(self.sam_whole, self.sam) and guards_intact(self.li_whole, self.li) and guards_intact(self.rl_whole, self.rl)


def call_dev(lib, ctx, d, counts, o, stream=None, null_sam=False):
    vp = ctypes.c_void_p
    inp = sam_input({k: (None if v is None else v.data_ptr()) for k, v in d.items() if k != "_keep"}, *counts)
    rep = _lib.SamReport()
    rc = lib.kiss_hip_fmi_sam_dev(ctx._ctx, ctypes.byref(inp), None if null_sam else vp(o.sam.data_ptr()), o.sam_cap,
                                  vp(o.li.data_ptr()) if o.want_lines else None, o.line_cap, vp(o.rl.data_ptr()), ctypes.byref(rep),
                                  vp(stream) if stream else None)
    return rc, rep


def u64_of(view):
    return view.cpu().numpy().view(np.uint64)


def same_as_model(want, o, rep, what):
    got = o.sam.cpu().numpy()[:len(want["sam"])].tobytes()
    if got != want["sam"]:
        k = next(i for i in range(len(got)) if got[i] != want["sam"][i])
        raise AssertionError("%s: sam differs at byte %d: got %r, want %r" % (what, k, got[max(0, k - 60):k + 40], want["sam"][max(0, k - 60):k + 40]))
    assert np.array_equal(u64_of(o.li), want["line_index"]), what
    assert np.array_equal(u64_of(o.rl), want["read_line"]), what
    assert {k: int(getattr(rep, k)) for k in REPORT} == want["report"], what
    assert o.intact(), what


@pytest.fixture(scope="module")
def gpu():
    import torch
    dev = torch.device("cuda", 0)
    ctx = kiss_amd.Context(max_n=1 << 22, device=0)
    yield _lib.load(), ctx, dev
    ctx.close()


def check(gpu, b, what, odd=False):
    lib, ctx, dev = gpu
    want = M.sam_model(b)
    arrs, counts = host_arrays(b)
    d = put(dev, arrs, odd)
    o = Outputs(dev, len(want["sam"]), want["report"]["lines"], counts[0], odd)
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0, (what, rc)
    same_as_model(want, o, rep, what)
    return want


# ---- the batches -----------------------------------------------------------------------------------------------------------
def shaped_batches():
    """(name, batch): the shapes at which the kernels change their path"""
    out = []
    r = rng_of(7)
    out.append(("lengths", M.make_batch(r, [1, 63, 64, 65, 300, 10000], [1, 2, 0, 1, 9, 1])))
    out.append(("lengths paired", M.make_batch(r, [1, 63, 64, 65, 300, 10000], [1, 2, 0, 1, 9, 1], paired=True)))
    names = [bytes(r.integers(33, 127, n).astype(np.uint8)) for n in (1, 63, 64, 65, 255)]
    out.append(("names", M.make_batch(r, [30] * 5, [1, 0, 2, 1, 3], names=names)))
    for md_len in (0, 1, 63, 64, 65, 1000):
        out.append(("md_len %d" % md_len, M.make_batch(r, [40, 50, 60, 70], [1, 2, 0, 3], paired=md_len % 2 == 1, md_len=md_len)))
    for n_ops in (1, 64, 65, 1000):
        out.append(("n_ops %d" % n_ops, M.make_batch(r, [3100, 3200], [2, 1], paired=n_ops == 65, n_ops=n_ops)))
    for paired in (False, True):
        out.append(("hits per read, paired %d" % paired, M.make_batch(r, [20, 33, 47, 150, 100, 64], [0, 1, 2, 9, 64, 65], paired=paired)))
    for Q in (1, 2, 63, 64, 65, 257):
        out.append(("Q %d" % Q, M.make_batch(r, r.integers(1, 80, Q), r.choice([0, 1, 2, 3], Q), paired=False)))
        if Q % 2 == 0:
            out.append(("Q %d paired" % Q, M.make_batch(r, r.integers(1, 80, Q), r.choice([0, 1, 2, 3], Q), paired=True)))
    for R in (0, 1, 3):
        for same in (False, True):
            out.append(("R %d same %d" % (R, same), M.make_batch(r, r.integers(20, 60, 8), [2] * 8, R=R, paired=True, same_names=same)))
    for paired in (False, True):
        for R in (0, 3):
            out.append(("big, paired %d R %d" % (paired, R), M.make_batch(r, r.integers(20, 60, 12), [3] * 12, R=R, paired=paired, big=True)))
    for chosen in ("first", "middle", "last", "none"):
        out.append(("chosen " + chosen, M.make_batch(r, r.integers(20, 60, 6), [3, 3, 1, 3, 0, 3], paired=True, chosen=chosen)))
    for qual in (False, True):
        for md in (False, True):
            for source in (False, True):
                out.append(("qual %d md %d source %d" % (qual, md, source),
                            M.make_batch(r, r.integers(20, 60, 6), [2, 1, 3, 0, 1, 2], paired=True, qual=qual, md=md, source=source)))
    return out


SHAPED = shaped_batches()


def test_the_first_200_random_batches(gpu):
    r = rng_of(20240)
    for k in range(200):
        check(gpu, M.random_batch(r), "random batch %d" % k)


@pytest.mark.parametrize("k", range(len(SHAPED)), ids=[n for n, _ in SHAPED])
def test_shapes(gpu, k):
    check(gpu, SHAPED[k][1], SHAPED[k][0])


def test_ten_thousand_one_hit_reads_beside_a_read_of_65_hits(gpu):
    r = rng_of(11)
    Q = 10001
    n_hits = np.ones(Q, np.int64)
    n_hits[5000] = 65
    want = check(gpu, M.make_batch(r, r.integers(30, 50, Q), n_hits, md=False), "10^4 reads")
    assert want["report"]["lines"] == 10000 + 65


def test_zero_reads(gpu):
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(3), [30], [1])
    arrs, _ = host_arrays(b)
    arrs["read_index"], arrs["hit_index"] = np.zeros(1, np.uint64), np.zeros(1, np.uint64)
    d = put(dev, arrs)
    o = Outputs(dev, 0, 0, 0)
    rc, rep = call_dev(lib, ctx, d, (0, 0, 3, 0), o)
    assert rc == 0 and u64_of(o.rl).tolist() == [0] and u64_of(o.li).tolist() == [0]
    assert {k: int(getattr(rep, k)) for k in REPORT} == dict.fromkeys(REPORT, 0)
    assert np.all(o.sam.cpu().numpy() == GUARD) and o.intact()


# ---- bad reads -------------------------------------------------------------------------------------------------------------
def bad_batch(kind, where):
    b = M.make_batch(rng_of(5), [30, 40, 50, 60, 70, 80, 90, 100], [2] * 8, R=3, paired=True, chosen="first")
    Q = 8
    q = {"first": 0, "middle": 3, "last": Q - 1}[where]
    h = int(b["hit_index"][q]) + 1
    a = int(b["hits"][h][M.H_ALN])
    C, L = len(b["alns"]), int(b["read_index"][q + 1]) - int(b["read_index"][q])
    if kind == "aln":
        b["hits"][h][M.H_ALN] = C
    elif kind == "ref":
        b["hits"][h][M.H_REF] = 3
    elif kind == "tbeg":
        b["hits"][h][M.H_REF] = 1
        b["alns"][a][M.A_TBEG] = int(b["bounds"][1]) - 1
    elif kind == "rbeg":
        b["alns"][a][M.A_RBEG] = int(b["alns"][a][M.A_REND]) + 1
    elif kind == "rend":
        b["alns"][a][M.A_REND] = L + 1
    elif kind == "bad_input":
        b["pairs"][q // 2][M.P_FLAGS] |= M.BAD_INPUT
    elif kind == "other_reads_hit":
        other = (q + 2) % Q
        b["pairs"][q // 2][M.P_HIT2 if q & 1 else M.P_HIT1] = int(b["hit_index"][other])
    return b, q


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kind", ["aln", "ref", "tbeg", "rbeg", "rend", "bad_input", "other_reads_hit"])
def test_bad_reads(gpu, kind, where):
    lib, ctx, dev = gpu
    b, q = bad_batch(kind, where)
    bad = M.bad_reads(b)
    assert q in bad and len(bad) == (2 if kind == "bad_input" else 1)
    want = M.sam_model(b)["report"]
    arrs, counts = host_arrays(b)
    o = Outputs(dev, 1 << 16, 64, counts[0])
    rc, rep = call_dev(lib, ctx, put(dev, arrs), counts, o)
    assert rc == _lib.KISS_HIP_E_INVALID
    assert (int(rep.bad), int(rep.first_bad)) == (want["bad"], want["first_bad"]) == (len(bad), bad[0])
    assert o.untouched() and o.intact()


# ---- size, then fill -------------------------------------------------------------------------------------------------------
def test_capacity_protocol(gpu):
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(9), [30, 40, 50, 60], [2, 0, 3, 1], paired=True)
    want = M.sam_model(b)
    total, lines = len(want["sam"]), want["report"]["lines"]
    arrs, counts = host_arrays(b)
    d = put(dev, arrs)
    totals = {k: want["report"][k] for k in ("lines", "sam_bytes", "unmapped_lines", "longest")}
    for sam_cap, line_cap, null_sam in ((0, 0, True), (total - 1, lines, False), (total, lines - 1, False), (0, lines, False)):
        o = Outputs(dev, sam_cap, line_cap, counts[0])
        rc, rep = call_dev(lib, ctx, d, counts, o, null_sam=null_sam)
        assert rc == _lib.KISS_HIP_E_INVALID, (sam_cap, line_cap)
        assert {k: int(getattr(rep, k)) for k in totals} == totals and rep.bad == 0
        assert o.untouched() and o.intact()
    # without line_index its capacity does not count; with room beyond the totals the fill stays inside them
    o = Outputs(dev, total, 0, counts[0], want_lines=False)
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0 and o.sam.cpu().numpy().tobytes() == want["sam"] and np.all(o.li.cpu().numpy() == GUARD) and o.intact()
    o = Outputs(dev, total + 100, lines + 5, counts[0])
    rc, rep = call_dev(lib, ctx, d, counts, o)
    assert rc == 0 and o.sam.cpu().numpy()[:total].tobytes() == want["sam"] and np.all(o.sam.cpu().numpy()[total:] == GUARD)
    assert np.array_equal(u64_of(o.li)[:lines + 1], want["line_index"]) and np.all(o.li.cpu().numpy()[8 * (lines + 1):] == GUARD) and o.intact()


def test_refused_arguments(gpu):
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(10), [30, 40, 50, 60], [2, 0, 3, 1], paired=True)
    arrs, counts = host_arrays(b)
    want = M.sam_model(b)

    def rc_of(change, counts=counts):
        a = dict(arrs)
        change(a)
        o = Outputs(dev, len(want["sam"]), want["report"]["lines"], counts[0])
        rc, _ = call_dev(lib, ctx, put(dev, a), counts, o)
        assert o.untouched() and o.intact()
        return rc

    for k in ("reads", "read_index", "names", "name_off", "name_len", "alns", "cigar", "cigar_index", "hits", "hit_index", "md_index", "ref_names",
              "ref_name_index", "bounds"):
        assert rc_of(lambda a, k=k: a.update({k: None})) == _lib.KISS_HIP_E_INVALID, k
    assert rc_of(lambda a: None, (3,) + counts[1:]) == _lib.KISS_HIP_E_INVALID  # Q odd with pairs

    def swapped(name, i):
        def change(a):
            x = a[name].copy()
            x[i], x[i + 1] = x[i + 1] + 1, x[i]
            a[name] = x
        return change

    for name in ("read_index", "hit_index", "cigar_index", "md_index", "ref_name_index"):
        assert rc_of(swapped(name, 1)) == _lib.KISS_HIP_E_INVALID, name

    def empty_read(a):
        x = a["read_index"].copy()
        x[2] = x[1]
        a["read_index"] = x
    assert rc_of(empty_read) == _lib.KISS_HIP_E_INVALID


# ---- alignment and stream ---------------------------------------------------------------------------------------------------
def test_odd_addresses(gpu):
    r = rng_of(13)
    check(gpu, M.make_batch(r, r.integers(1, 200, 40), r.choice([0, 1, 2, 5], 40), paired=True), "odd addresses, paired", odd=True)
    check(gpu, M.make_batch(r, r.integers(1, 200, 33), r.choice([0, 1, 2, 5], 33)), "odd addresses", odd=True)


def test_work_runs_on_the_callers_stream_and_is_done_on_return(gpu):
    """the pattern of tests/test_dev_stream_gpu.py: a decoy batch of the same shapes lies in the inputs; a delay on the caller's
    stream, and behind it the copies that put the real batch back; the call, made while the stream is busy, must see the real
    one and be finished on return"""
    import time
    import torch
    from tests.test_dev_stream_gpu import Delayed, caller_stream
    lib, ctx, dev = gpu
    b = M.make_batch(rng_of(17), rng_of(18).integers(30, 200, 64), [2] * 64, paired=True)
    want = M.sam_model(b)
    arrs, counts = host_arrays(b)
    decoy = dict(arrs)
    decoy["reads"] = (arrs["reads"] + 1) % 6
    decoy["qual"] = 33 + (arrs["qual"] - 33 + 1) % 94
    decoy["md"] = arrs["md"][::-1].copy()
    d = put(dev, arrs)
    changed = ("reads", "qual", "md")  # (lines of the same lengths, other bytes)
    staging = {k: d[k].clone() for k in changed}
    o = Outputs(dev, len(want["sam"]), want["report"]["lines"], counts[0])
    for _ in range(2):  # warm up on the null stream; the second call is the idle duration
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc, rep = call_dev(lib, ctx, d, counts, o)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0
    same_as_model(want, o, rep, "warm-up on the null stream")
    for k in changed:
        d[k].copy_(torch.from_numpy(np.ascontiguousarray(decoy[k]).reshape(-1).view(np.uint8).copy()))
    o.sam.fill_(GUARD)
    o.li.fill_(GUARD)
    o.rl.fill_(GUARD)
    torch.cuda.synchronize()
    rc, rep = call_dev(lib, ctx, d, counts, o)  # (the decoy gives other bytes)
    assert rc == 0 and o.sam.cpu().numpy()[:len(want["sam"])].tobytes() != want["sam"]
    o.sam.fill_(GUARD)
    torch.cuda.synchronize()
    s = caller_stream()
    with Delayed(s, idle_ms) as delay:
        for k in changed:
            d[k].copy_(staging[k], non_blocking=True)
    assert not s.query(), "the stream was idle at the moment of the call"
    rc, rep = call_dev(lib, ctx, d, counts, o, stream=s.cuda_stream)
    got = o.sam.cpu().numpy().tobytes()  # (a copy on the null stream, which does not wait for s)
    delay.check("kiss_hip_fmi_sam_dev")
    assert rc == 0 and got == want["sam"]
    same_as_model(want, o, rep, "on the caller's stream")


# ---- the host entry ----------------------------------------------------------------------------------------------------------
def test_the_host_entry_gives_the_same_bytes():
    picked = [b for _, b in SHAPED[::4]][:12]
    assert len(picked) == 12
    for k, b in enumerate(picked):
        want = M.sam_model(b)
        got = kiss_amd.sam_writer.sam_lines(**b)
        assert got["sam"].tobytes() == want["sam"], k
        assert np.array_equal(got["line_index"], want["line_index"]) and np.array_equal(got["read_line"], want["read_line"]), k
        assert {x: got["report"][x] for x in REPORT} == want["report"], k
    b, _ = bad_batch("rend", "middle")
    with pytest.raises(_lib.KissHipError) as e:
        kiss_amd.sam_writer.sam_lines(**b)
    assert e.value.status == _lib.KISS_HIP_E_INVALID and (e.value.report["bad"], e.value.report["first_bad"]) == (1, 3)


# ---- placement across 2^31 and 2^32 (the supposed cause of the first writer's fault) -----------------------------
def test_arrays_on_both_sides_of_2_31_and_across_2_32(gpu):
    """every array of the batch is valid memory wherever it lies, so a correct kernel cannot fault here; a kernel that widens
    the low half of an address with its sign would"""
    import torch
    lib, ctx, dev = gpu
    r = rng_of(23)
    names = [bytes(r.integers(33, 127, 200).astype(np.uint8)) for _ in range(8)]
    b = M.make_batch(r, [300] * 8, [2] * 8, paired=True, names=names, md_len=150)
    want = M.sam_model(b)
    arrs, counts = host_arrays(b)
    total = len(want["sam"])
    assert min(arrs[k].size for k in ("reads", "names", "md")) > 1024 and total > 1024
    G = 1 << 32
    arena = torch.empty(G + (64 << 20), dtype=torch.uint8, device=dev)
    base = arena.data_ptr()
    to_carry = (-base) % G  # the offset of the first multiple of 2^32 in the arena
    high = (to_carry + (1 << 31) + 4096) % G
    places = {"high half": high if high >= PAD else high + G, "low half": to_carry + 4096,
              "across a multiple of 2^32": to_carry - 1024 if to_carry >= 1024 + PAD else to_carry + G - 1024}
    for what, off in places.items():
        lo = (base + off) & (G - 1)
        assert {"high half": lo >= 1 << 31, "low half": lo < 1 << 31, "across a multiple of 2^32": lo == G - 1024}[what]
        assert off >= PAD and off + total + PAD <= arena.numel()
        for name in ("sam", "reads", "names", "md"):
            if name == "sam":
                whole = arena[off - PAD:off + total + PAD]
                whole.fill_(GUARD)
                d = put(dev, arrs)
                o = Outputs(dev, total, want["report"]["lines"], counts[0], sam_view=(whole, whole[PAD:PAD + total]))
            else:
                d = put(dev, arrs, place={name: arena[off:]})
                o = Outputs(dev, total, want["report"]["lines"], counts[0])
            rc, rep = call_dev(lib, ctx, d, counts, o)
            assert rc == 0, (what, name)
            same_as_model(want, o, rep, "%s at %s" % (name, what))
    del arena
