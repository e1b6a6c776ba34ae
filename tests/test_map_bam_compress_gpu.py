"""bam_compress=True beside bam=True in FMIndex.map, map_pairs and kiss_amd.batches.map_file, and write_bam(compress=True): the
blocks are compressed on the device (kiss_hip_bgzf_deflate_dev) and decompress to exactly what the blocks of the
same call without bam_compress decompress to; every other key of the result is what it was."""
import gzip

import pytest

from tests import bam_model as B
from tests.test_fm_md_gpu import same_results
from tests.test_fm_mm_gpu import TEXTS, text
from tests.test_map_bam_gpu import records_for
from tests.test_map_sam_gpu import quals_of

pytestmark = pytest.mark.gpu

CODING = ("stored_blocks", "fixed_blocks", "dynamic_blocks", "literals", "matches", "match_bytes")


def same_but_compressed(packed, stored):
    """two results of one call, with and without bam_compress -> the decompressed bytes"""
    raw = gzip.decompress(stored["bam"]) if stored["bam"] else b""
    assert (gzip.decompress(packed["bam"]) if packed["bam"] else b"") == raw
    assert packed.keys() - stored.keys() == {"bam_block_index"}
    same_results({k: v for k, v in packed.items() if k not in ("bam", "bam_report", "bam_block_index", "qual")},
                 {k: v for k, v in stored.items() if k not in ("bam", "bam_report", "qual")})
    rp, rs = packed["bam_report"], stored["bam_report"]
    assert {k: rp[k] for k in rs if not k.startswith("ms_") and k != "out_bytes"} == {k: rs[k] for k in rs if not k.startswith("ms_") and k != "out_bytes"}
    assert rp["out_bytes"] == len(packed["bam"]) <= rs["out_bytes"] and set(CODING) <= rp.keys() and not set(CODING) & rs.keys()
    assert rp["stored_blocks"] + rp["fixed_blocks"] + rp["dynamic_blocks"] == rp["blocks"] and rp["literals"] + rp["match_bytes"] == len(raw)
    index = packed["bam_block_index"].tolist()
    assert len(index) == rp["blocks"] + 1 and index[0] == 0 and index[-1] == len(packed["bam"]) and index == sorted(index)
    for b in range(rp["blocks"]):   # every block is a gzip member of its own
        assert gzip.decompress(packed["bam"][index[b]:index[b + 1]]) == raw[b * 65280:(b + 1) * 65280]
    return raw


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_bam_compress(name):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    records = records_for(S.size)
    if records is None:
        return
    common = dict(both_strands=True, chain_params=dict(min_score=25, band=100), names=["read%d/x" % q for q in range(len(reads))],
                  qual=quals_of(reads, 5), want_md=True)
    stored = f.map(reads, S, 15, 0, 200, bam=True, **common, **records)
    packed = f.map(reads, S, 15, 0, 200, bam=True, bam_compress=True, **common, **records)
    raw = same_but_compressed(packed, stored)
    if len(raw) > 4000:
        assert len(packed["bam"]) < len(stored["bam"])
    with pytest.raises(ValueError):
        f.map(reads, S, 15, 0, 200, bam_compress=True, **common, **records)


@pytest.mark.parametrize("rescue", [None, True])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_bam_compress(name, rescue):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    records = records_for(S.size)
    if records is None:
        return
    m1, m2 = mates_of(name)
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue, want_md=bool(rescue),
                  names=["pair:%d" % p for p in range(len(m1))], qual=(quals_of(m1, 6), quals_of(m2, 7)))
    stored = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, **common, **records)
    packed = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, bam_compress=True, **common, **records)
    same_but_compressed(packed, stored)


def test_map_file_and_write_bam_compressed(tmp_path_factory):
    import kiss_amd.bam_writer as W
    from kiss_amd.batches import map_file
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_bam_compress")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq", "stored.bam", "packed.bam")}
    write_fastq(paths["s1.fq"], s1, "/1", 1)
    write_fastq(paths["s2.fq"], s2, "/2", 2)
    single = [r for pair in zip(s1, s2) for r in pair]
    write_fastq(paths["single.fq"], single, "", 3)
    f = truth_index(S)
    try:
        n, Q, P = S.size, len(single), len(s1)
        records = dict(bounds=[0, n // 3, n], ref_names=["one", "two"])
        head = W.bam_header(records["ref_names"], records["bounds"], "X")
        for what, files, count, kw in (("single", (paths["single.fq"], None), Q, dict(both_strands=True, want_md=True)),
                                       ("paired", (paths["s1.fq"], paths["s2.fq"]), P, dict(rescue=True, want_md=True, **LIBRARY))):
            for batch_reads in (1, 7, count + 1):
                stored = list(map_file(f, files[0], S, files[1], batch_reads=batch_reads, bam=True, **kw, **records))
                packed = list(map_file(f, files[0], S, files[1], batch_reads=batch_reads, bam=True, bam_compress=True, **kw, **records))
                assert len(stored) == len(packed) == -(-count // batch_reads), what
                for a, b in zip(packed, stored):
                    same_but_compressed(a, b)
            a = W.write_bam(paths["stored.bam"], f, files[0], S, files[1], batch_reads=7, version="X", **kw, **records)
            b = W.write_bam(paths["packed.bam"], f, files[0], S, files[1], batch_reads=7, version="X", compress=True, **kw, **records)
            blob, small = open(paths["stored.bam"], "rb").read(), open(paths["packed.bam"], "rb").read()
            assert small.endswith(B.BGZF_EOF) and b["bytes"] == len(small) < len(blob) == a["bytes"] and (a["batches"], a["records"]) == (b["batches"], b["records"])
            got_head, got = B.skip_header(gzip.decompress(small))
            assert (got_head, got) == B.skip_header(gzip.decompress(blob)) and got_head == head, what
            assert len(B.split_records(got)) == b["records"]
        with pytest.raises(ValueError):
            list(map_file(f, paths["single.fq"], S, batch_reads=7, both_strands=True, bam_compress=True))
    finally:
        f.close()
