"""bam_sort=True beside bam=True in FMIndex.map and map_pairs, and write_bam(sort=True): the records of the batch, or of the whole
file, are put into coordinate order on the device (kiss_hip_bam_sort_dev) between the record call and the framing.
The decompressed records are tests/bam_sort_model.py's sort of the records of the same call without bam_sort, bam_order connects
bam_read_rec to the sorted slots, every other key of the result is what it was, map_file refuses the option, and a sorted file does
not depend on how it was cut into batches."""
import gzip

import numpy as np
import pytest

from tests import bam_model as B
from tests import bam_sort_model as M
from tests.test_fm_md_gpu import same_results
from tests.test_fm_mm_gpu import TEXTS, text
from tests.test_map_bam_gpu import records_for
from tests.test_map_sam_gpu import quals_of

pytestmark = pytest.mark.gpu

SORT_KEYS = ("unplaced", "ms_sort_total", "ms_sort_key", "ms_sort", "ms_sort_copy")


def model_sort(raw, n_ref):
    """unframed records -> the model's result for them"""
    recs = B.split_records(raw)
    bam, ri = M.pack(recs)
    return recs, (M.sort if len(recs) <= 300 else M.sort_fast)(bam, ri, n_ref)


def same_but_sorted(ordered, plain, n_ref):
    """two results of one call, with and without bam_sort"""
    raw = gzip.decompress(plain["bam"]) if plain["bam"] else b""
    got = gzip.decompress(ordered["bam"]) if ordered["bam"] else b""
    recs, want = model_sort(raw, n_ref)
    assert got == want["bam"].tobytes()
    assert B.split_records(got) == [recs[r] for r in want["order"]]
    assert ordered.keys() - plain.keys() == {"bam_order"}
    assert np.array_equal(ordered["bam_order"], want["order"]) and ordered["bam_order"].dtype == np.uint32
    assert np.array_equal(ordered["bam_rec_index"], want["rec_index"]) and np.array_equal(plain["bam_rec_index"], M.pack(recs)[1])
    # bam_read_rec counts the records as they were written; bam_order says where each of them went
    assert np.array_equal(ordered["bam_read_rec"], plain["bam_read_rec"])
    slot_of = np.zeros(len(recs), np.int64)
    slot_of[ordered["bam_order"].astype(np.int64)] = np.arange(len(recs))
    idx = ordered["bam_rec_index"]
    for q in range(len(plain["bam_read_rec"]) - 1):
        for r in range(int(plain["bam_read_rec"][q]), int(plain["bam_read_rec"][q + 1])):
            s = int(slot_of[r])
            assert got[int(idx[s]):int(idx[s + 1])] == recs[r]
    skip = ("bam", "bam_report", "bam_rec_index", "bam_order", "bam_block_index", "qual")
    same_results({k: v for k, v in ordered.items() if k not in skip}, {k: v for k, v in plain.items() if k not in skip})
    ro, rp = ordered["bam_report"], plain["bam_report"]
    assert set(ro) - set(rp) == set(SORT_KEYS) and ro["unplaced"] == want["report"]["unplaced"]
    same = lambda rep: {k: rep[k] for k in rp if not k.startswith("ms_") and k not in  # noqa: E731
                        ("out_bytes", "stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches", "match_bytes")}
    assert same(ro) == same(rp)
    return want


@pytest.mark.parametrize("compress", [False, True], ids=["stored", "compressed"])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_bam_sort(name, compress):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    records = records_for(S.size)
    if records is None:
        return
    common = dict(both_strands=True, chain_params=dict(min_score=25, band=100), names=["read%d/x" % q for q in range(len(reads))],
                  qual=quals_of(reads, 5), want_md=True, bam_compress=compress)
    plain = f.map(reads, S, 15, 0, 200, bam=True, **common, **records)
    ordered = f.map(reads, S, 15, 0, 200, bam=True, bam_sort=True, **common, **records)
    same_but_sorted(ordered, plain, len(records["ref_names"]))
    with pytest.raises(ValueError):
        f.map(reads, S, 15, 0, 200, bam_sort=True, **{k: v for k, v in common.items() if k != "bam_compress"}, **records)


@pytest.mark.parametrize("compress", [False, True], ids=["stored", "compressed"])
@pytest.mark.parametrize("rescue", [None, True])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_bam_sort(name, rescue, compress):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    records = records_for(S.size)
    if records is None:
        return
    m1, m2 = mates_of(name)
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue, want_md=bool(rescue),
                  names=["pair:%d" % p for p in range(len(m1))], qual=(quals_of(m1, 6), quals_of(m2, 7)), bam_compress=compress)
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, **common, **records)
    ordered = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, bam_sort=True, **common, **records)
    same_but_sorted(ordered, plain, len(records["ref_names"]))


def test_map_file_refuses_and_write_bam_sorts_the_whole_file(tmp_path_factory):
    import kiss_amd.bam_writer as W
    from kiss_amd.batches import map_file
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_bam_sort")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq", "plain.bam", "sorted.bam", "never.bam")}
    write_fastq(paths["s1.fq"], s1, "/1", 1)
    write_fastq(paths["s2.fq"], s2, "/2", 2)
    single = [r for pair in zip(s1, s2) for r in pair]
    write_fastq(paths["single.fq"], single, "", 3)
    f = truth_index(S)
    try:
        n, Q, P = S.size, len(single), len(s1)
        records = dict(bounds=[0, n // 3, n], ref_names=["one", "two"])
        head = W.bam_header(records["ref_names"], records["bounds"], "X", sort_order="coordinate")
        assert head != W.bam_header(records["ref_names"], records["bounds"], "X")
        with pytest.raises(ValueError, match="write_bam"):
            list(map_file(f, paths["single.fq"], S, batch_reads=7, both_strands=True, bam=True, bam_sort=True, **records))
        # ins_min / ins_max given: the pairs do not depend on the batch the insert size would be estimated from
        for what, files, count, kw in (("single", (paths["single.fq"], None), Q, dict(both_strands=True, want_md=True)),
                                       ("paired", (paths["s1.fq"], paths["s2.fq"]), P, dict(rescue=True, want_md=True, **LIBRARY))):
            a = W.write_bam(paths["plain.bam"], f, files[0], S, files[1], batch_reads=7, version="X", **kw, **records)
            plain_head, plain = B.skip_header(gzip.decompress(open(paths["plain.bam"], "rb").read()))
            assert plain_head == W.bam_header(records["ref_names"], records["bounds"], "X") and "sort_report" not in a
            recs, want = model_sort(plain, 2)
            assert want["order"].tolist() != list(range(len(recs)))  # (there is something to sort)
            for compress in (False, True):
                seen = set()
                for batch_reads in (1, 7, count, count + 1):
                    b = W.write_bam(paths["sorted.bam"], f, files[0], S, files[1], batch_reads=batch_reads, version="X", sort=True, compress=compress,
                                    **kw, **records)
                    blob = open(paths["sorted.bam"], "rb").read()
                    assert blob.endswith(B.BGZF_EOF) and b["bytes"] == len(blob) and b["records"] == a["records"] == len(recs), what
                    assert b["batches"] == -(-count // batch_reads)
                    raw = gzip.decompress(blob)
                    got_head, got = B.skip_header(raw)
                    assert got_head == head and got == want["bam"].tobytes(), (what, batch_reads, compress)
                    rep = b["sort_report"]
                    assert {k: rep[k] for k in want["report"]} == want["report"]
                    seen.add(raw)
                assert len(seen) == 1  # byte-identical across the batch sizes
                if compress:
                    assert len(blob) < a["bytes"]
    finally:
        f.close()


def test_write_bam_names_the_bytes_when_the_device_cannot_hold_them(tmp_path, monkeypatch):
    """the allocation of the sorted copy fails (torch's own error, raised in the place of bam_sort_dev): MemoryError with the bytes
    asked for, and nothing written to the path"""
    import torch
    import kiss_amd.bam_writer as W
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    from tests.test_map_file_gpu import write_fastq
    S, m1, m2, _ = insert_truth_case(200, 10)
    write_fastq(str(tmp_path / "r.fq"), m1[:6], "", 3)
    f = truth_index(S)
    try:
        def no_room(*a, **k):
            raise torch.cuda.OutOfMemoryError("no room")
        monkeypatch.setattr(W, "bam_sort_dev", no_room)
        out = tmp_path / "never.bam"
        with pytest.raises(MemoryError, match=r"\d+ bytes"):
            W.write_bam(str(out), f, str(tmp_path / "r.fq"), S, batch_reads=4, version="X", sort=True, both_strands=True,
                        bounds=[0, S.size // 3, S.size], ref_names=["one", "two"])
        assert not out.exists()
    finally:
        f.close()
