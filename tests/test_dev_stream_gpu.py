"""Which stream the work of a device entry runs on, and when the entry returns.

include/kiss_hip.h: `stream` is the caller's hipStream_t, the call's work is ordered behind what the caller has queued on
it, and the call returns after that work has completed.  Torch's streams are non-blocking: nothing on the null stream or
on the ctx's own stream waits for them.  So for every entry that takes a stream (tests/dev_cases.py):

  1. warm up: the case runs on the NULL stream with the real input on the ctx, so that every pool and work array has its
     size (kiss_hip_ctx_workspace_bytes does not move over the timed call: a hipFree inside it would wait for the device
     and hide what is looked for);
  2. every device input is overwritten with a DECOY, another valid input of the same shapes whose every output differs;
  3. on s = torch.cuda.Stream(): a delay, and behind it the copies that put the REAL input back;
  4. while s is still busy the entry is called with s;
  5. on return, without any torch synchronisation, the outputs are read with kiss_hip_copy_to_host (a blocking copy on the
     null stream, which does not wait for s) and held against the model's answer for the real input.

A launch, memset, copy or host-side fetch that the library issues anywhere but on s before its first synchronisation sees
the decoy; a call that returns before its work is done is read half finished.  The decoy is valid data: reading it gives a
wrong answer, not a wild address.

Checked up to their first hipFree only: kiss_hip_fmi_build_dev, kiss_hip_fmi_build_ex_dev, kiss_hip_fmi8_build_dev and
kiss_hip_ctx_verify_sa_dev allocate and free scratch of their own inside every call (not pooled, not counted by
kiss_hip_ctx_workspace_bytes), and a hipFree waits for the caller's stream too; what these entries launch behind their first
free is not held to the stream rule by this file.

Two conditions keep a test from passing vacuously, and both are asserted: s was busy at the moment of the call, and the
delay, measured with events on s, was at least ten times the call's own duration on an idle device and at least 20 ms.

The last test is about what a ctx does AFTER such a call: it keeps no caller's stream."""
import ctypes
import time

import numpy as np
import pytest

from tests import dev_cases, dev_place, dev_run

pytestmark = pytest.mark.gpu

CASES = dev_cases.CASES
STREAM_CASES = [c for c in CASES if c.in_stream_test]
MIN_DELAY_MS, DELAY_FACTOR, MAX_DELAY_MS = 20.0, 10.0, 3000.0
PROBE_CYCLES = 20_000_000

_calibration = {}


def calibrate():
    """how long torch.cuda._sleep spins per cycle on this device (measured once, with two events); if it does not spin at
    all, a chain of matrix products is the delay instead"""
    import torch
    if _calibration:
        return _calibration
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    e[0].record()
    torch.cuda._sleep(PROBE_CYCLES)
    e[1].record()
    e[1].synchronize()
    sleep_ms = e[0].elapsed_time(e[1])
    _calibration["sleep_probe_ms"] = sleep_ms
    if sleep_ms >= 1.0:
        _calibration["cycles_per_ms"] = PROBE_CYCLES / sleep_ms
    else:
        a = torch.randn(2048, 2048, device=dev_run.device())
        torch.mm(a, a)
        torch.cuda.synchronize()
        e[2].record()
        for _ in range(8):
            a2 = torch.mm(a, a)
        e[3].record()
        e[3].synchronize()
        _calibration["matrix"] = a
        _calibration["mm_ms"] = e[2].elapsed_time(e[3]) / 8
        del a2
    print("delay calibration: %r" % {k: v for k, v in _calibration.items() if k != "matrix"})
    return _calibration


def queue_delay(ms):
    """a delay of about `ms` milliseconds on the current stream"""
    import torch
    cal = calibrate()
    assert ms <= MAX_DELAY_MS, "a delay of %.0f ms: the call is too slow for this test" % ms
    if "cycles_per_ms" in cal:
        torch.cuda._sleep(int(ms * cal["cycles_per_ms"]))
    else:
        for _ in range(int(ms / cal["mm_ms"]) + 1):
            torch.mm(cal["matrix"], cal["matrix"])


def caller_stream():
    """The caller's stream: non-blocking, as every torch stream, and of HIGH priority.  The runtime keeps a few hardware queues
    per priority and spreads the streams of that priority over them; torch alone creates 32 streams of each.  Two streams
    that share a hardware queue wait for each other whatever the library does, so a caller's stream of the ctx's own
    priority would, now and then, hide a launch on the wrong stream (it would wait for the delay like a right one) and hold
    up the ctx's own work in the last test.  A stream of another priority shares no queue with the null stream or with the
    ctx's own stream."""
    import torch
    return torch.cuda.Stream(priority=-1)


class Delayed:
    """with Delayed(s, idle_ms) as d: queue the delay on s ...; d.check() afterwards waits for s and asserts the delay's size"""

    def __init__(self, stream, idle_ms):
        import torch
        calibrate()
        self.s, self.idle_ms = stream, idle_ms
        self.need_ms = max(MIN_DELAY_MS, DELAY_FACTOR * idle_ms)
        self.e0, self.e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        self.ctx = torch.cuda.stream(stream)

    def __enter__(self):
        self.ctx.__enter__()
        self.e0.record(self.s)
        queue_delay(1.5 * self.need_ms + 5.0)
        self.e1.record(self.s)
        return self

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)

    def check(self, what):
        self.s.synchronize()
        self.ms = self.e0.elapsed_time(self.e1)
        print("STREAM %-58s idle call %8.3f ms, delay %8.1f ms" % (what, self.idle_ms, self.ms))
        assert self.ms >= self.need_ms, "%s: the delay was %.1f ms, the call alone takes %.3f ms" % (what, self.ms, self.idle_ms)


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c.id for c in STREAM_CASES])
def test_work_runs_on_the_callers_stream_and_is_done_on_return(case):
    import torch
    from kiss_amd import _lib
    lib = _lib.load()
    real, decoy = case.data("real"), case.data("decoy")
    # the decoy is another input of the same shapes, and the model says that every compared output differs
    for name, arr in real.inp.items():
        assert decoy.inp[name].shape == arr.shape and decoy.inp[name].dtype == arr.dtype, (case.id, name)
        assert name in case.constant or not np.array_equal(decoy.inp[name], arr), (case.id, name)
    wr, wd = case.normalise(real.outs, real.host), case.normalise(decoy.outs, decoy.host)
    for name in real.outs:
        sl_r, sl_d = case.defined(name, real.host), case.defined(name, decoy.host)
        assert name in case.constant or not np.array_equal(wr[name][sl_r], wd[name][sl_d]), (case.id, name)
    for k in getattr(case, "must_differ", ()):
        assert real.scal[k] != decoy.scal[k], (case.id, k)
    assert real.outs or getattr(case, "must_differ", ()), case.id
    s = caller_stream()
    with dev_run.context(case) as ctx:
        ins, outs, p = dev_run.put(case, real, 0x00)
        staging = {name: v.clone() for name, v in ins.items()}
        # 1. warm up on the NULL stream; the second call is the idle duration
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            scal = case.call(lib, ctx._ctx, p, real.host, None)
            torch.cuda.synchronize()
            idle_ms = (time.perf_counter() - t0) * 1e3
        dev_run.check(case, real, dev_run.fetch_outputs(lib, outs), scal, "warm-up on the NULL stream")
        # 2. the decoy in every input, the outputs as they were before any call
        for name, v in ins.items():
            if v.numel():
                v.copy_(torch.from_numpy(decoy.inp[name].reshape(-1).view(np.uint8).copy()))
        for v in outs.values():
            v.fill_(0xEE)
        torch.cuda.synchronize()
        before = ctx.workspace_bytes()
        # 3. a delay on s, and behind it the real input
        with Delayed(s, idle_ms) as delay:
            for name, v in ins.items():
                if v.numel():
                    v.copy_(staging[name], non_blocking=True)
        # 4. the call, while s is busy
        assert not s.query(), "the stream was idle at the moment of the call"
        scal = case.call(lib, ctx._ctx, p, real.host, s.cuda_stream)
        # 5. no torch synchronisation: a blocking copy on the null stream
        raw = dev_run.fetch_outputs(lib, outs)
        after = ctx.workspace_bytes()
        delay.check(case.id)
        assert after == before, "the timed call allocated work arrays (%d -> %d bytes): the warm-up did not size them" % (before, after)
        dev_run.check(case, real, raw, scal, "on the caller's stream")
        dev_place.check_canaries(*outs.values())
        dev_place.check_canaries(*ins.values())


# ---- what the ctx does after the call ---------------------------------------------------------------------------------------
def same_counts(counts, hist):
    """count[c] and lms_count[c] of {count[c], s_type_count[c], lms_count[c]} against the oracle's get_lms histogram (the two
    groups tests/test_suffix_sort_gpu.py compares)"""
    counts = [int(x) for x in counts]
    return counts[0:4] == hist[4, :4].tolist() and counts[8:12] == hist[2, :4].tolist()


AFTER_CALL = ("get_stats", "stage_outputs", "local_lms", "reserve", "scan", "null_sort")


@pytest.fixture(scope="module")
def after_call_steps(oracle):
    """name -> (what the ctx runs on s just before, the entry that takes no stream), and s"""
    import torch
    from kiss_amd import _lib
    lib = _lib.load()
    dev = dev_run.device()
    vp = ctypes.c_void_p
    n, k = 20003, 256
    S = dev_cases.dna_text(n, 10)
    want_sa, want_sorted = oracle.suffix_sort(S, k, stages=True)
    want_asc, hist = oracle.get_lms(S)
    want_asc = want_asc[:-1]
    want_sorted = want_sorted[1:]
    m = int(want_asc.size)
    small = dev_cases.dna_text(1000, 3)
    rng = np.random.default_rng(5)
    scan_in = rng.integers(0, 1 << 20, 10000).astype(np.uint32)
    scan_want = (np.concatenate([[0], np.cumsum(scan_in.astype(np.int64))[:-1]]) & 0xFFFFFFFF).astype(np.uint32)
    d_S = torch.from_numpy(S).to(dev)
    d_SA = torch.zeros(n + 1, dtype=torch.int32, device=dev)
    d_small = torch.from_numpy(small).to(dev)
    d_small_SA = torch.zeros(1001, dtype=torch.int32, device=dev)
    d_keys = torch.zeros(m + 8, dtype=torch.int64, device=dev)
    d_pos = torch.zeros(m + 8, dtype=torch.int32, device=dev)
    s = caller_stream()

    def sort_on_s(ctx):
        rc = lib.kiss_hip_ctx_suffix_sort_dna_u32_dev(ctx._ctx, vp(d_S.data_ptr()), n, k, 0, vp(d_SA.data_ptr()), vp(s.cuda_stream))
        assert rc == 0 and np.array_equal(d_SA.cpu().numpy().view(np.uint32), want_sa)

    def classify_on_s(ctx):
        counts = (ctypes.c_uint64 * 13)()
        rc = lib.kiss_hip_stage_classify(ctx._ctx, vp(d_S.data_ptr()), n, k, 0, n, ctypes.byref(counts), vp(s.cuda_stream))
        assert rc == 0 and same_counts(counts, hist) and counts[12] <= m
        d_keys.fill_(-1)
        d_pos.fill_(-1)

    def get_stats(ctx):
        st = _lib.Stats()
        assert lib.kiss_hip_get_stats(ctx._ctx, ctypes.byref(st)) == 0
        assert (st.n, st.m, st.k) == (n, m, k), (st.n, st.m, st.k)

    def stage_outputs(ctx):
        asc, srt, counts = np.zeros(m, np.uint32), np.zeros(m, np.uint32), np.zeros(12, np.uint64)
        assert lib.kiss_hip_ctx_get_stage_outputs(ctx._ctx, vp(asc.ctypes.data), vp(srt.ctypes.data), vp(counts.ctypes.data)) == 0
        assert np.array_equal(asc, want_asc) and np.array_equal(srt, want_sorted) and same_counts(counts, hist)

    def local_lms(ctx):
        ml, mf = ctypes.c_uint64(), ctypes.c_uint64()
        rc = lib.kiss_hip_stage_local_lms(ctx._ctx, vp(d_keys.data_ptr()), vp(d_pos.data_ptr()), ctypes.byref(ml), ctypes.byref(mf))
        assert rc == 0 and ml.value == m and mf.value <= m
        # the copy is the ctx's own list (kiss_hip_stage_view), entry for entry, and that list holds the LMS suffixes of the text
        got_keys, got_pos = np.zeros(m + 8, np.uint64), np.zeros(m + 8, np.uint32)
        assert lib.kiss_hip_copy_to_host(vp(got_keys.ctypes.data), vp(d_keys.data_ptr()), got_keys.nbytes) == 0
        assert lib.kiss_hip_copy_to_host(vp(got_pos.ctypes.data), vp(d_pos.data_ptr()), got_pos.nbytes) == 0
        own_keys, own_pos = np.zeros(m, np.uint64), np.zeros(m, np.uint32)
        for which, out in ((_lib.VIEW_LOCAL_KEYS, own_keys), (_lib.VIEW_LOCAL_POS, own_pos)):
            ptr, cap = vp(), ctypes.c_uint64()
            assert lib.kiss_hip_stage_view(ctx._ctx, which, ctypes.byref(ptr), ctypes.byref(cap)) == 0 and cap.value >= m
            assert lib.kiss_hip_copy_to_host(vp(out.ctypes.data), ptr, out.nbytes) == 0
        assert np.array_equal(got_keys[:m], own_keys) and np.array_equal(got_pos[:m], own_pos)
        assert (got_keys[m:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (got_pos[m:] == 0xFFFFFFFF).all()
        assert np.array_equal(np.sort(got_pos[:m]), want_asc)

    def reserve(ctx):
        cap = ctypes.c_uint64()
        ptr = vp()
        assert lib.kiss_hip_stage_view(ctx._ctx, _lib.VIEW_SORTED, ctypes.byref(ptr), ctypes.byref(cap)) == 0
        want = min(2 * int(cap.value), ctx.max_n // 2)
        assert want > cap.value
        assert lib.kiss_hip_stage_reserve(ctx._ctx, want) == 0
        assert lib.kiss_hip_stage_view(ctx._ctx, _lib.VIEW_SORTED, ctypes.byref(ptr), ctypes.byref(cap)) == 0 and cap.value >= want

    def scan(ctx):
        data = scan_in.copy()
        assert lib.kiss_hip_debug_scan_u32(ctx._ctx, vp(data.ctypes.data), data.size) == 0
        assert np.array_equal(data, scan_want)

    def null_sort(ctx):
        rc = lib.kiss_hip_ctx_suffix_sort_dna_u32_dev(ctx._ctx, vp(d_small.data_ptr()), 1000, k, 0, vp(d_small_SA.data_ptr()), None)
        got = np.zeros(1001, np.uint32)
        assert rc == 0 and lib.kiss_hip_copy_to_host(vp(got.ctypes.data), vp(d_small_SA.data_ptr()), got.nbytes) == 0
        assert np.array_equal(got, oracle.suffix_sort(small, k))

    steps = dict(get_stats=(sort_on_s, get_stats), stage_outputs=(sort_on_s, stage_outputs), local_lms=(classify_on_s, local_lms),
                 reserve=(sort_on_s, reserve), scan=(sort_on_s, scan), null_sort=(sort_on_s, null_sort))
    assert tuple(steps) == AFTER_CALL
    return steps, s


@pytest.mark.parametrize("name", AFTER_CALL)
def test_a_ctx_does_not_keep_the_callers_stream_past_the_call(after_call_steps, name):
    """After a call on s has returned, s belongs to the caller again.  With a delay queued on s, every entry of the ctx that
    takes no stream -- kiss_hip_get_stats, kiss_hip_ctx_get_stage_outputs, kiss_hip_stage_local_lms in its copy form after a
    kiss_hip_stage_classify on s, kiss_hip_stage_reserve with a capacity that forces regrowth, kiss_hip_debug_scan_u32, a sort
    on the NULL stream -- gives the right data and returns while s is still busy: it neither queued its work behind the delay
    nor waited for it."""
    import torch
    import kiss_amd
    steps, s = after_call_steps
    before, entry = steps[name]
    # the entry's own duration on an idle device, on a ctx of its own (a regrowth happens once per ctx)
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        before(ctx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        entry(ctx)
        torch.cuda.synchronize()
        idle_ms = (time.perf_counter() - t0) * 1e3
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        before(ctx)
        torch.cuda.synchronize()
        with Delayed(s, idle_ms) as delay:
            pass
        assert not s.query()
        entry(ctx)
        busy = not s.query()
        delay.check("after %s: %s" % (before.__name__, entry.__name__))
        assert busy, "%s waited for the caller's stream, or queued its work on it" % entry.__name__


# ---- kiss_hip_stage_reserve: the arrays it replaces -----------------------------------------------------------------------------
def _view_capacity(lib, ctx):
    from kiss_amd import _lib
    ptr, cap = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.kiss_hip_stage_view(ctx._ctx, _lib.VIEW_SORTED, ctypes.byref(ptr), ctypes.byref(cap)) == 0
    return int(cap.value)


def _null_sort_is_right(lib, ctx, oracle):
    import torch
    S = dev_cases.dna_text(1000, 3)
    d_S = torch.from_numpy(S).to(dev_run.device())
    d_SA = torch.zeros(1001, dtype=torch.int32, device=dev_run.device())
    rc = lib.kiss_hip_ctx_suffix_sort_dna_u32_dev(ctx._ctx, ctypes.c_void_p(d_S.data_ptr()), 1000, 256, 0, ctypes.c_void_p(d_SA.data_ptr()), None)
    assert rc == 0 and np.array_equal(d_SA.cpu().numpy().view(np.uint32), oracle.suffix_sort(S, 256))


def test_arrays_a_reserve_replaces_are_held_until_the_next_call_with_a_stream_and_counted(oracle):
    """hipFree waits for every stream of the device, so kiss_hip_stage_reserve leaves the arrays it replaces to the next call
    that takes a stream.  Until then kiss_hip_ctx_workspace_bytes counts old and new arrays; afterwards the new ones alone."""
    import kiss_amd
    from kiss_amd import _lib
    lib = _lib.load()
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        _null_sort_is_right(lib, ctx, oracle)
        cap0, ws0 = _view_capacity(lib, ctx), ctx.workspace_bytes()
        want = min(2 * cap0, ctx.max_n // 2)
        assert want > cap0 and lib.kiss_hip_stage_reserve(ctx._ctx, want) == 0
        ws1 = ctx.workspace_bytes()
        assert _view_capacity(lib, ctx) >= want and ctx.workspace_bytes() == ws1  # (asking for the views frees nothing)
        _null_sort_is_right(lib, ctx, oracle)
        ws2 = ctx.workspace_bytes()
        assert ws0 < ws2 < ws1, (ws0, ws1, ws2)
        assert _view_capacity(lib, ctx) >= want
        assert lib.kiss_hip_stage_reserve(ctx._ctx, want) == 0 and ctx.workspace_bytes() == ws2  # (large enough: nothing moves)


def test_a_reserve_that_does_not_fit_beside_the_old_arrays_frees_them_first_and_fails_cleanly(oracle):
    """the hooks build's allocation limit (kiss_hip_debug_fail_alloc_over) fails the regrowth twice: beside the old arrays, then
    after they were freed.  KISS_HIP_E_NOMEM, nothing half allocated, and the ctx sorts again once there is room."""
    import kiss_amd
    from kiss_amd import _lib
    lib = _lib.load(True)
    with kiss_amd.Context(max_n=1 << 20, hooks=True) as ctx:
        _null_sort_is_right(lib, ctx, oracle)
        cap0 = _view_capacity(lib, ctx)
        want = min(2 * cap0, ctx.max_n // 2)
        assert lib.kiss_hip_debug_fail_alloc_over(ctx._ctx, 1 << 20) == 0
        assert lib.kiss_hip_stage_reserve(ctx._ctx, want) == _lib.KISS_HIP_E_NOMEM
        held = ctx.workspace_bytes()
        assert lib.kiss_hip_debug_fail_alloc_over(ctx._ctx, 0) == 0
        _null_sort_is_right(lib, ctx, oracle)
        assert ctx.workspace_bytes() > held  # (the default reservation is back)
        assert lib.kiss_hip_stage_reserve(ctx._ctx, want) == 0 and _view_capacity(lib, ctx) >= want
