"""FMIndex.map(bam=True), map_pairs(bam=True), kiss_amd.batches.map_file(bam=True) and kiss_amd.bam_writer.write_bam: the BGZF
blocks of a batch, written and framed on the device from the buffers the stages left there.  Decompressed and decoded by
tests/bam_model.py, the records are the SAM lines of the same call, line for line; the records of a file mapped in batches are
the records of the whole file; without bam every result is what it was."""
import gzip

import numpy as np
import pytest

from tests import bam_model as B
from tests.test_fm_mm_gpu import TEXTS, text
from tests.test_map_sam_gpu import REF_NAMES, quals_of

pytestmark = pytest.mark.gpu

BAM_KEYS = {"bam", "bam_rec_index", "bam_read_rec", "bam_report"}


def records_of(res):
    """the blocks of a result -> its records, held against the index arrays and the report"""
    assert isinstance(res["bam"], bytes)
    raw = gzip.decompress(res["bam"]) if res["bam"] else b""
    recs = B.split_records(raw)
    rep = res["bam_report"]
    assert (rep["records"], rep["bam_bytes"], rep["out_bytes"]) == (len(recs), len(raw), len(res["bam"])) and rep["bad"] == 0
    assert res["bam_rec_index"].tolist() == np.concatenate(([0], np.cumsum([len(r) for r in recs]))).tolist()
    assert int(res["bam_read_rec"][-1]) == len(recs) and rep["blocks"] == -(-len(raw) // 65280)
    assert res["bam"] == B.frame(raw)
    return raw, recs


def same_as_the_sam_lines(res, ref_names):
    raw, recs = records_of(res)
    names = [x.encode() for x in ref_names]
    assert [B.bam_to_sam(r, names) for r in recs] == res["sam"].splitlines(keepends=True)
    assert np.array_equal(res["bam_read_rec"], res["sam_read_line"]) and res["bam_report"]["unmapped_records"] == res["sam_report"]["unmapped_lines"]
    return raw


def records_for(n):
    """bam needs records: two where the text has two bases, one where it has one, none for the text of no base"""
    if n >= 2:
        return dict(bounds=[0, n // 2, n], ref_names=REF_NAMES)
    return dict(bounds=[0, n], ref_names=REF_NAMES[:1]) if n else None


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_bam_gives_the_sam_lines_as_records(name):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_md_gpu import same_results
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    records = records_for(S.size)
    common = dict(both_strands=True, chain_params=dict(min_score=25, band=100))
    if records is None:
        with pytest.raises(ValueError):
            f.map(reads, S, 15, 0, 200, bam=True, ref_names=REF_NAMES[:1], **common)
        return
    qual = quals_of(reads, 5)
    names = ["read%d/x" % (q * q) for q in range(len(reads))]
    for k, given in enumerate((dict(), dict(names=names, qual=qual, want_md=True))):
        res = f.map(reads, S, 15, 0, 200, sam=True, bam=True, **given, **common, **records)
        same_as_the_sam_lines(res, records["ref_names"])
        only = f.map(reads, S, 15, 0, 200, bam=True, **given, **common, **records)
        assert only["bam"] == res["bam"] and "sam" not in only
        plain = f.map(reads, S, 15, 0, 200, **{x: v for x, v in dict(given, **common, bounds=records["bounds"]).items() if x not in ("names", "qual")})
        assert not BAM_KEYS & plain.keys()
        same_results({x: v for x, v in only.items() if x not in BAM_KEYS}, plain)
    for wrong in (dict(want_cigar=False, **records), dict(ref_names=records["ref_names"]), dict(bounds=records["bounds"])):
        with pytest.raises(ValueError):
            f.map(reads, S, bam=True, **wrong)


@pytest.mark.parametrize("rescue", [None, True])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_bam_gives_the_sam_lines_as_records(name, rescue):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    records = records_for(S.size)
    if records is None:
        return  # (the text of no base: test_map_with_bam... holds the refusal)
    m1, m2 = mates_of(name)
    q1, q2 = quals_of(m1, 6), quals_of(m2, 7)
    names = ["pair:%d" % p for p in range(len(m1))]
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue, want_md=bool(rescue))
    res = f.map_pairs(m1, m2, S, 15, 0, 200, sam=True, bam=True, names=names, qual=(q1, q2), **common, **records)
    raw = same_as_the_sam_lines(res, records["ref_names"])
    assert (b"YRC\1" in raw) == (b"YR:i:1" in res["sam"]) and (b"YTZCP\0" in raw) == (b"YT:Z:CP" in res["sam"])
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, **common, bounds=records["bounds"])
    assert not BAM_KEYS & plain.keys()


def test_map_file_and_write_bam_give_the_records_of_the_whole_file(tmp_path_factory):
    import kiss_amd.bam_writer as W
    from kiss_amd.batches import map_file
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_bam")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq", "out.bam")}
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
            whole = list(map_file(f, files[0], S, files[1], batch_reads=count + 1, sam=True, bam=True, **kw, **records))
            assert len(whole) == 1
            raw = same_as_the_sam_lines(whole[0], records["ref_names"])
            assert len(raw) > 2000
            for batch_reads in (1, 7, count):
                got = list(map_file(f, files[0], S, files[1], batch_reads=batch_reads, bam=True, **kw, **records))
                assert len(got) == -(-count // batch_reads) and not any("sam" in x for x in got), what
                assert b"".join(records_of(x)[0] for x in got) == raw, (what, batch_reads)
                assert gzip.decompress(b"".join(x["bam"] for x in got)) == raw
            # the whole file: header, batches, end-of-file block
            done = W.write_bam(paths["out.bam"], f, files[0], S, files[1], batch_reads=7, version="X", **kw, **records)
            blob = open(paths["out.bam"], "rb").read()
            assert blob.endswith(B.BGZF_EOF) and blob.startswith(B.frame(head)) and done["bytes"] == len(blob)
            assert done["batches"] == -(-count // 7) and done["records"] == len(B.split_records(raw))
            assert B.skip_header(gzip.decompress(blob)) == (head, raw), what
        with pytest.raises(ValueError):
            W.write_bam(paths["out.bam"], f, paths["single.fq"], S, ref_names=["one", "two"])
        plain = list(map_file(f, paths["single.fq"], S, batch_reads=7, both_strands=True))
        assert not any(BAM_KEYS & x.keys() for x in plain)
    finally:
        f.close()
