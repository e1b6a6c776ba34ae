"""write_bam(sort=True, bai=...): the BAI index of the whole sorted file, built on the device (kiss_hip_bai_dev)
from the arrays the file is framed from.  The .bai is tests/bai_model.py's index of the records and blocks found in the file itself,
a reader that goes through it (the model's fetch, with zlib) gets exactly the records that overlap a region, the index does not
depend on how the reads were cut into batches, the .bam is byte for byte the one written without the option, and the option is
refused where it has no meaning.  Stored and compressed, on the read files of tests/test_map_bam_sort_gpu.py and on the text
families of the map tests."""
import gzip
import io
import os

import pytest

from tests import bai_model as M
from tests import bam_model as B
from tests import bam_sort_model as SM
from tests.test_fm_mm_gpu import TEXTS, text
from tests.test_map_bam_gpu import records_for

pytestmark = pytest.mark.gpu

COUNTS = ("records", "bam_bytes", "bai_bytes", "chunks", "bins", "windows", "mapped", "unmapped_placed", "no_coor", "bad", "first_bad")


def check_index(blob, bai, bounds, report=None):
    """the index of the file `blob` is the model's, and a reader finds through it what overlaps; -> the records"""
    n_ref = len(bounds) - 1
    head, body = B.skip_header(gzip.decompress(blob))
    recs = B.split_records(body)
    bam, ri = SM.pack(recs)
    base, block_index = M.file_frame(blob, len(head))
    want = M.build(bam, ri, n_ref, 0, block_index, base)
    assert want["status"] == "ok" and bai == want["bai"]
    if report is not None:
        assert {k: report[k] for k in COUNTS} == want["report"]
    parsed = M.parse(bai)
    reader = M.BgzfReader(blob)
    found = 0
    for ref in range(n_ref):
        L = int(bounds[ref + 1]) - int(bounds[ref])
        grid = [(0, L), (L - 1, L), (0, 1), (L // 2, L // 2 + 1), (L // 3, 2 * L // 3)] + [(w << 14, min(L, (w + 1) << 14)) for w in range(-(-L // 16384))]
        grid += [((1 << 14) - 1, (1 << 14) + 1), ((1 << 17) - 1, 1 << 17)]
        for rec in recs[::max(1, len(recs) // 8)]:
            r, b, e, _, _ = M.interval(rec)
            if r == ref:
                grid += [(b, b + 1), (e - 1, e), (e, e + 1), (max(0, b - 1), b)]
        for beg, end in grid:
            if 0 <= beg < end:
                got = M.fetch(reader, parsed, ref, beg, end)
                assert got == M.overlapping(recs, ref, beg, end), (ref, beg, end)
                found += len(got)
    assert found or not any(M.interval(r)[0] >= 0 for r in recs)
    return recs


def test_write_bam_with_an_index(tmp_path_factory):
    import kiss_amd.bam_writer as W
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_bam_index")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq", "plain.bam", "indexed.bam", "other.bai", "never.bam")}
    write_fastq(paths["s1.fq"], s1, "/1", 1)
    write_fastq(paths["s2.fq"], s2, "/2", 2)
    single = [r for pair in zip(s1, s2) for r in pair]
    write_fastq(paths["single.fq"], single, "", 3)
    f = truth_index(S)
    try:
        n, Q, P = S.size, len(single), len(s1)
        records = dict(bounds=[0, n // 3, n], ref_names=["one", "two"])
        for what, files, count, kw in (("single", (paths["single.fq"], None), Q, dict(both_strands=True, want_md=True)),
                                       ("paired", (paths["s1.fq"], paths["s2.fq"]), P, dict(rescue=True, want_md=True, **LIBRARY))):
            for compress in (False, True):
                a = W.write_bam(paths["plain.bam"], f, files[0], S, files[1], batch_reads=7, version="X", sort=True, compress=compress, **kw, **records)
                assert "bai_bytes" not in a and "bai_report" not in a and not os.path.exists(paths["plain.bam"] + ".bai")
                plain = open(paths["plain.bam"], "rb").read()
                seen = set()
                for batch_reads in (1, 7, count, count + 1):
                    for p in (paths["indexed.bam"], paths["indexed.bam"] + ".bai"):
                        if os.path.exists(p):
                            os.remove(p)
                    b = W.write_bam(paths["indexed.bam"], f, files[0], S, files[1], batch_reads=batch_reads, version="X", sort=True, compress=compress,
                                    bai=True, **kw, **records)
                    blob, bai = open(paths["indexed.bam"], "rb").read(), open(paths["indexed.bam"] + ".bai", "rb").read()
                    assert blob == plain, (what, compress, batch_reads)              # the .bam is what it was
                    assert b["bai_bytes"] == len(bai) and {k: v for k, v in b.items() if not k.startswith("bai_")}.keys() == a.keys()
                    recs = check_index(blob, bai, records["bounds"], b["bai_report"])
                    assert len(recs) == b["records"] and b["bai_report"]["records"] == len(recs)
                    seen.add(bai)
                assert len(seen) == 1                                                # the same index however the reads were cut
                # a name and a file object for the index; a file object for the file
                b = W.write_bam(paths["indexed.bam"], f, files[0], S, files[1], batch_reads=7, version="X", sort=True, compress=compress,
                                bai=paths["other.bai"], **kw, **records)
                assert open(paths["other.bai"], "rb").read() == bai
                to, to_bai = io.BytesIO(), io.BytesIO()
                W.write_bam(to, f, files[0], S, files[1], batch_reads=7, version="X", sort=True, compress=compress, bai=to_bai, **kw, **records)
                assert to.getvalue() == plain and to_bai.getvalue() == bai
        with pytest.raises(ValueError, match="sort=True"):
            W.write_bam(paths["never.bam"], f, paths["single.fq"], S, batch_reads=7, version="X", bai=True, both_strands=True, **records)
        with pytest.raises(ValueError, match="file name"):
            W.write_bam(io.BytesIO(), f, paths["single.fq"], S, batch_reads=7, version="X", sort=True, bai=True, both_strands=True, **records)
        assert not os.path.exists(paths["never.bam"]) and not os.path.exists(paths["never.bam"] + ".bai")
    finally:
        f.close()


@pytest.mark.parametrize("compress", [False, True], ids=["stored", "compressed"])
@pytest.mark.parametrize("name", sorted(n for n in TEXTS if n != "n0"))  # (the text of no base has no reference: no BAM file of it)
def test_the_index_of_the_text_families(name, compress, tmp_path):
    import kiss_amd.bam_writer as W
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    records = records_for(S.size)
    assert records is not None
    with open(str(tmp_path / "r.fq"), "w") as o:  # (codes above 3 are no-bases)
        for q, r in enumerate(reads):
            o.write("@r%d\n%s\n+\n%s\n" % (q, "".join("ACGTN"[min(int(c), 4)] for c in r), "I" * len(r)))
    path = str(tmp_path / "t.bam")
    b = W.write_bam(path, f, str(tmp_path / "r.fq"), S, batch_reads=max(1, len(reads) // 3), version="X", sort=True, compress=compress, bai=True,
                    both_strands=True, chain_params=dict(min_score=25, band=100), **records)
    recs = check_index(open(path, "rb").read(), open(path + ".bai", "rb").read(), records["bounds"], b["bai_report"])
    assert len(recs) == b["records"] >= len(reads)
