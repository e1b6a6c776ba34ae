"""tests/dev_place.py on CPU tensors: offsets, sizes, guard contents, and that a write one byte outside a view is seen.
Also, without a GPU: the device entries that tests/test_dev_placement_gpu.py and tests/test_dev_stream_gpu.py run are exactly
the *_dev functions of include/kiss_hip.h that take a stream, so an entry added later without these tests fails here."""
import os
import re

import numpy as np
import pytest

from tests import dev_place as dp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fill", (0x00, 0xFF, (1, 2)))
@pytest.mark.parametrize("lead,guard,dtype,count", ((1, 64, np.uint8, 4099), (3, 300, np.uint8, 1), (4, 256, np.uint32, 33),
                                                    (8, 1, np.uint64, 7), (0, 0, np.uint8, 5), (255, 512, np.uint8, 257)))
def test_offsets_sizes_and_guard_contents(lead, guard, dtype, count, fill):
    rng = np.random.default_rng(count)
    a = rng.integers(0, 200, count).astype(dtype)
    v = dp.place(a, lead, guard, fill)
    p = v.placement
    assert p.store.data_ptr() % 256 == 0
    assert v.data_ptr() % 256 == lead and v.data_ptr() == p.store.data_ptr() + p.offset == p.address
    assert v.numel() == a.nbytes == p.nbytes and v.dtype.itemsize == 1
    assert np.array_equal(dp.read_back(v, dtype), a)
    img = p.store.numpy()
    assert p.offset >= guard and img.size - (p.offset + p.nbytes) >= guard
    pattern = (fill,) if isinstance(fill, int) else fill
    outside = np.concatenate([np.arange(p.offset), np.arange(p.offset + p.nbytes, img.size)])
    assert np.array_equal(img[outside], np.asarray(pattern, np.uint8)[outside % len(pattern)])
    dp.check_canaries(v)


def test_the_alternating_fill_differs_from_both_plain_fills_in_the_low_two_bits():
    a = np.zeros(16, np.uint8)
    lows = [dp.place(a, 1, 64, f).placement.store.numpy()[:64] & 3 for f in (0x00, 0xFF, (1, 2))]
    assert (lows[0] != lows[2]).all() and (lows[1] != lows[2]).all() and (lows[0] != lows[1]).all()


@pytest.mark.parametrize("where", ("before", "behind", "far_before", "last_byte_of_the_allocation"))
@pytest.mark.parametrize("fill", (0x00, 0xFF, (1, 2)))
def test_a_write_one_byte_outside_the_view_is_detected(where, fill):
    v = dp.place_out(40, 4, 128, fill)
    p = v.placement
    at = {"before": p.offset - 1, "behind": p.offset + p.nbytes, "far_before": 0,
          "last_byte_of_the_allocation": p.store.numel() - 1}[where]
    dp.check_canaries(v)
    p.store[at] = int(p.store[at]) ^ 0x10
    with pytest.raises(AssertionError, match="canary"):
        dp.check_canaries(v)


def test_writes_inside_the_view_trip_nothing():
    v = dp.place_out(40, 8, 64, 0xFF)
    assert (dp.read_back(v) == 0xEE).all()
    v[:] = 7
    v[0] = 1
    v[-1] = 2
    dp.check_canaries(v)
    got = dp.read_back(v)
    assert got[0] == 1 and got[-1] == 2 and (got[1:-1] == 7).all()


def test_an_empty_array_still_has_its_place():
    v = dp.place(np.zeros(0, np.uint32), 4, 64, 0)
    assert v.numel() == 0 and v.placement.offset % 256 == 4 and v.placement.address % 256 == 4
    dp.check_canaries(v)


def test_the_leads_are_what_the_header_promises():
    """every array of every case at the alignment of its element and no more; every byte array -- texts, reads, patterns,
    raw bytes, bwt and occ2 of the DNA index -- at lead 1 in one of the two placements and at lead 3 in the other; the one
    array that owes more (the 16-byte aligned bwt of the byte index) at 16"""
    from tests import dev_cases
    seen = set()
    for case in dev_cases.CASES:
        data = case.data("real")
        for name, arr in list(data.inp.items()) + list(data.outs.items()):
            leads = [case.lead(name, arr, flip) for flip in (0, 1)]
            if name in case.leads:
                assert (case.entry, name, leads) in (("kiss_hip_fmi8_build_dev", "bwt", [16, 16]), ("kiss_hip_fmi8_query_dev", "bwt", [16, 16]))
            elif arr.dtype.itemsize == 1:
                assert sorted(leads) == [1, 3], (case.id, name, leads)
                seen.add(name)
            else:
                assert leads == [arr.dtype.itemsize] * 2, (case.id, name, leads)
    assert {"S", "text", "reads", "patterns", "raw", "bwt", "occ2", "map", "mismatches"} <= seen
    # a C caller that points into a loaded .fmi: bwt of the DNA queries at lead 1 in the first placement
    for case in dev_cases.CASES:
        if case.entry in ("kiss_hip_fmi_query_batch_dev", "kiss_hip_fmi_query_ex_dev", "kiss_hip_fmi_query_mm_dev", "kiss_hip_fmi_seeds_dev"):
            assert case.lead("bwt", case.data("real").inp["bwt"], 0) == 1, case.id


# ---- the list of entries --------------------------------------------------------------------------------------------------
# out of scope by decision (the issue of these tests): kiss_hip_multi_* run on the ctx's own streams (kiss_amd/multi_gpu.py)
OUT_OF_SCOPE = {"kiss_hip_multi_suffix_sort_dna_u32_dev"}


def dev_entries_with_a_stream():
    text = open(os.path.join(ROOT, "include", "kiss_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    out = []
    for m in re.finditer(r"\bint\s+(kiss_hip_\w+_dev)\s*\(([^;{]*)\)\s*;", text):
        if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)):
            out.append(m.group(1))
    return out


def test_every_device_entry_with_a_stream_has_a_placement_and_a_stream_case():
    from tests import dev_cases
    header = set(dev_entries_with_a_stream()) - OUT_OF_SCOPE
    assert len(header) >= 20 and "kiss_hip_fmi_aln_merge_dev" in header and "kiss_hip_ctx_verify_sa_dev" in header
    covered = {c.entry for c in dev_cases.CASES}
    assert covered == header, (sorted(header - covered), sorted(covered - header))
    # both GPU files parametrise over that very list
    from tests import test_dev_placement_gpu, test_dev_stream_gpu
    assert test_dev_placement_gpu.CASES is dev_cases.CASES and test_dev_stream_gpu.CASES is dev_cases.CASES
    assert not (OUT_OF_SCOPE & covered)
