"""Where the caller's arrays lie.  Every device entry that takes a stream (tests/dev_cases.py) runs one small case four ways:
the ordinary way, every array at the start of an allocation of its own, and six times with every input `lead` bytes past
a 256-byte boundary (tests/dev_place.py: everything at the alignment of its element and no more, a byte array at 1 AND at
3: Case.lead's flip, three runs each) between guard bands of 0x00, of 0xFF and of 01 02 01 02 ... .  Outputs are views of
exactly the capacity the entry is told, between canary bands.

Expected: all seven results equal the model or the oracle element by element, return code, totals and report fields
included; the six guarded runs are bit-identical, so no result depends on a byte outside an input; no canary is touched,
so nothing is written outside an output.  Guards are memory of the same allocation: a stray access cannot fault.

Where the header demands more than the element's alignment -- the 16-byte aligned bwt of the byte index -- the demand is
tested instead: KISS_HIP_E_INVALID before anything is launched, no output changed."""
import numpy as np
import pytest

from tests import dev_cases, dev_place, dev_run

pytestmark = pytest.mark.gpu

CASES = dev_cases.CASES


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_result_does_not_depend_on_where_the_arrays_lie(case):
    from kiss_amd import _lib
    lib = _lib.load()
    data = case.data("real")
    guarded = []
    with dev_run.context(case) as ctx:
        for fill, flip in [(None, 0)] + [(f, flip) for flip in (0, 1) for f in dev_run.FILLS]:
            where = "the ordinary way" if fill is None else "at the leads (byte arrays %s), guards %r" % (("1 3 1 ..", "3 1 3 ..")[flip], fill)
            ins, outs, p = dev_run.put(case, data, fill, flip)
            scal = case.call(lib, ctx._ctx, p, data.host, None)
            raw = dev_run.fetch_outputs(lib, outs)
            dev_run.check(case, data, raw, scal, where)
            dev_place.check_canaries(*outs.values())
            if fill is not None:
                dev_place.check_canaries(*ins.values())  # (and no input was written to)
                for name, v in ins.items():
                    assert np.array_equal(dev_place.read_back(v), data.inp[name].reshape(-1).view(np.uint8)), (case.id, name)
                guarded.append((raw, scal))
    for raw, scal in guarded[1:]:
        assert scal == guarded[0][1], (case.id, scal, guarded[0][1])
        for name in raw:
            assert np.array_equal(raw[name], guarded[0][0][name]), "%s: %s depends on the bytes around the inputs" % (case.id, name)


def fm8_case(entry):
    return next(c for c in CASES if c.entry == entry and c.in_stream_test)


@pytest.mark.parametrize("lead", (1, 4, 8))
@pytest.mark.parametrize("entry", ("kiss_hip_fmi8_build_dev", "kiss_hip_fmi8_query_dev"))
def test_the_byte_index_refuses_a_bwt_that_is_not_16_byte_aligned(entry, lead):
    """include/kiss_hip.h: bwt of kiss_hip_fmi8_view is 16-byte aligned (its rows are read 16 at a time); anything else is
    KISS_HIP_E_INVALID -- decided from the address alone, so nothing is launched and no output changes"""
    from kiss_amd import _lib
    lib = _lib.load()
    case = fm8_case(entry)
    data = case.data("real")
    with dev_run.context(case) as ctx:
        ins, outs, p = dev_run.put(case, data, 0xFF)
        where = outs if "bwt" in outs else ins
        moved = dev_place.place(data.outs["bwt"] if "bwt" in outs else data.inp["bwt"], lead, dev_run.GUARD, 0xFF, device=dev_run.device())
        where["bwt"] = moved
        p["bwt"] = moved.placement.address
        assert p["bwt"] % 16 == lead
        before = {name: dev_place.read_back(v) for name, v in outs.items()}
        scal = case.call(lib, ctx._ctx, p, data.host, None)
        assert scal["rc"] == _lib.KISS_HIP_E_INVALID, scal
        for name, v in outs.items():
            assert np.array_equal(dev_place.read_back(v), before[name]), name
        dev_place.check_canaries(*outs.values())
        # and the same arrays with bwt where the header wants it: the model's answer
        good = dev_place.place(data.outs["bwt"] if "bwt" in outs else data.inp["bwt"], 16, dev_run.GUARD, 0xFF, device=dev_run.device())
        if "bwt" in outs:
            good[:] = 0xEE
        where["bwt"] = good
        p["bwt"] = good.placement.address
        scal = case.call(lib, ctx._ctx, p, data.host, None)
        dev_run.check(case, data, dev_run.fetch_outputs(lib, outs), scal, "bwt at 16")


# ---- the one 16-byte load of a caller's array that only a large sort reaches -----------------------------------------------
@pytest.mark.parametrize("lead", (4, 8, 16))
@pytest.mark.parametrize("which", ("u8", "dna_doubling_over_the_suffix_array"))
def test_the_binned_inverse_reads_a_suffix_array_at_any_4_byte_address(which, lead, monkeypatch, oracle):
    """isa.hip builds the inverse of the caller's d_SA (the byte sort, and the exact DNA order when the doubling runs over the
    whole suffix array) with 16-byte loads once the array is past 2^25 entries.  The header asks 4 bytes of d_SA, so the wide
    loads are taken only where the address allows.  The hooks build takes that path at test size (KISS_HIP_ISA_DIRECT_MAX);
    d_SA at 4, 8 and 16 bytes past a 256-byte boundary, between canaries, against the models."""
    import kiss_amd
    from kiss_amd import _lib
    from tests import fm8_model
    lib = _lib.load(True)
    monkeypatch.setenv("KISS_HIP_ISA_DIRECT_MAX", "1000")
    n = 20003
    if which == "u8":
        raw = fm8_model.english_like(n, 3)
        S, want = np.frombuffer(raw, np.uint8), fm8_model.exact_sa_doubling(raw)
    else:
        monkeypatch.setenv("KISS_HIP_NO_LMS_EXACT", "1")
        S = dev_cases.dna_text(n, 77)
        want = oracle.suffix_sort(S, dev_cases.K_UNBOUNDED)
    dev = dev_run.device()
    d_S = dev_place.place(S, 3, dev_run.GUARD, (1, 2), device=dev)
    d_SA = dev_place.place_out(4 * (n + 1), lead, dev_run.GUARD, 0xFF, device=dev)
    vp = dev_cases.VP
    with kiss_amd.Context(max_n=1 << 20, hooks=True) as ctx:
        if which == "u8":
            rc = lib.kiss_hip_ctx_suffix_sort_u8_dev(ctx._ctx, vp(d_S.placement.address), n, vp(d_SA.placement.address), None)
        else:
            rc = lib.kiss_hip_ctx_suffix_sort_dna_u32_dev(ctx._ctx, vp(d_S.placement.address), n, dev_cases.K_UNBOUNDED,
                                                          _lib.ALGO_PREFIX_DOUBLING, vp(d_SA.placement.address), None)
        held = ctx.workspace_bytes()
    assert rc == 0
    assert held >= 2 * (8 << 24), held  # (the two pair arrays of the partition passes: the direct scatter has none)
    assert np.array_equal(dev_place.read_back(d_SA, np.uint32), want)
    dev_place.check_canaries(d_SA, d_S)
