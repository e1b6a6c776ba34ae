"""bam_markdup=True beside bam=True in FMIndex.map and map_pairs, and write_bam(sort=True, markdup=True): the duplicate templates of
the batch, or of the whole file, get FLAG 0x400 on the device (kiss_hip_bam_markdup_dev) between the record call and
the sort.  The flags are tests/markdup_model.py's on the records of the same call without the option and every other byte and key is
what it was; a read file with planted copies is marked exactly where they were planted; a marked file does not depend on how it was
cut into batches, differs from the unmarked one only in bytes 18 - 19 of records and has the same index; map_file and the unsorted
write_bam refuse the option."""
import gzip
import struct

import numpy as np
import pytest

from tests import bam_model as B
from tests import bam_sort_model as SM
from tests import markdup_model as M
from tests.test_fm_md_gpu import same_results
from tests.test_fm_mm_gpu import TEXTS, text
from tests.test_map_bam_gpu import records_for
from tests.test_map_sam_gpu import quals_of

pytestmark = pytest.mark.gpu

COUNTS = ("records", "templates", "pairs", "fragments", "unmapped_templates", "ambiguous", "dup_pairs", "dup_fragments", "dup_records", "bad",
          "first_bad")
NEW_KEYS = {"bam_dup", "bam_markdup_report"}


def model_mark(raw, n_ref, min_qual=15):
    """unframed records -> their list and the model's result for them"""
    recs = B.split_records(raw)
    bam, ri = M.join(recs)
    return recs, M.markdup_model(bam, ri, n_ref, min_qual, decide=M.duplicates_by_loops if len(recs) <= 300 else M.duplicates_by_dicts)


def same_but_marked(marked, plain, n_ref, min_qual=15):
    """two results of one call, with and without bam_markdup"""
    raw = gzip.decompress(plain["bam"]) if plain["bam"] else b""
    got = gzip.decompress(marked["bam"]) if marked["bam"] else b""
    recs, want = model_mark(raw, n_ref, min_qual)
    assert got == want["bam"].tobytes()
    assert marked.keys() - plain.keys() == NEW_KEYS
    assert marked["bam_dup"].dtype == np.uint8 and np.array_equal(marked["bam_dup"], want["dup"])
    assert {k: marked["bam_markdup_report"][k] for k in COUNTS} == want["report"]
    skip = ("bam", "bam_report", "qual") + tuple(NEW_KEYS)
    same_results({k: v for k, v in marked.items() if k not in skip}, {k: v for k, v in plain.items() if k not in skip})
    same = lambda rep: {k: v for k, v in rep.items() if not k.startswith("ms_")}  # noqa: E731
    assert same(marked["bam_report"]) == same(plain["bam_report"])
    return recs, want


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_bam_markdup(name):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    records = records_for(S.size)
    if records is None:
        return
    reads = list(reads) + list(reads)  # every read twice, under another name: the second one of a mapped read is a duplicate
    quals = quals_of(reads, 5)
    common = dict(both_strands=True, chain_params=dict(min_score=25, band=100), names=["read%d/x" % q for q in range(len(reads))], qual=quals,
                  want_md=True)
    n_ref = len(records["ref_names"])
    plain = f.map(reads, S, 15, 0, 200, bam=True, **common, **records)
    marked = f.map(reads, S, 15, 0, 200, bam=True, bam_markdup=True, **common, **records)
    recs, want = same_but_marked(marked, plain, n_ref)
    mapped = sum(1 for t in want["templates"] if t["cls"] == "fragment")
    assert want["report"]["dup_fragments"] >= mapped // 2 and (mapped == 0 or want["report"]["dup_records"] > 0)
    # another threshold; and with the sort behind it: the marked records in coordinate order, bam_dup still as they were written
    low = f.map(reads, S, 15, 0, 200, bam=True, bam_markdup=dict(min_qual=60), **common, **records)
    same_but_marked(low, plain, n_ref, 60)
    both = f.map(reads, S, 15, 0, 200, bam=True, bam_markdup=True, bam_sort=True, bam_compress=True, **common, **records)
    bam, ri = SM.pack(B.split_records(want["bam"].tobytes()))
    ordered = (SM.sort if len(recs) <= 300 else SM.sort_fast)(bam, ri, n_ref)
    assert gzip.decompress(both["bam"]) == ordered["bam"].tobytes() if both["bam"] else not recs
    assert np.array_equal(both["bam_dup"], want["dup"]) and np.array_equal(both["bam_order"], ordered["order"])
    with pytest.raises(ValueError):
        f.map(reads, S, 15, 0, 200, bam_markdup=True, **common, **records)


@pytest.mark.parametrize("rescue", [None, True])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_bam_markdup(name, rescue):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    records = records_for(S.size)
    if records is None:
        return
    m1, m2 = mates_of(name)
    m1, m2 = list(m1) + list(m1), list(m2) + list(m2)
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue, want_md=bool(rescue),
                  names=["pair:%d" % p for p in range(len(m1))], qual=(quals_of(m1, 6), quals_of(m2, 7)))
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, **common, **records)
    marked = f.map_pairs(m1, m2, S, 15, 0, 200, bam=True, bam_markdup=True, **common, **records)
    _, want = same_but_marked(marked, plain, len(records["ref_names"]))
    whole = want["report"]["pairs"] + want["report"]["fragments"]
    assert want["report"]["dup_pairs"] + want["report"]["dup_fragments"] >= whole // 2


# ---- a read file with planted copies ---------------------------------------------------------------------------------------------
def planted_files(tmp, pairs, singles, copies=3):
    """`pairs` pairs of the truth case `copies` times each, under names of their own and with a quality of their own (which copy
    has the best one changes from pair to pair), and `singles` pairs whose first mate is that of a planted pair, with the best
    quality of all, and whose second mate maps nowhere -> text, the two paths, the single-end path, the names that must be marked"""
    from tests.test_fm_insert_gpu import insert_truth_case
    S, m1, m2, _ = insert_truth_case(pairs, 0)
    rng = np.random.default_rng(77)
    letters = lambda r: "".join("ACGT"[int(c)] for c in r)  # noqa: E731
    entries, marked = [], set()
    for k in range(copies):
        for p in range(pairs):
            q = 20 + 10 * ((p + k) % copies)  # 20, 30, 40: the copy with 40 stays
            name = "p%d.copy%d" % (p, k)
            entries.append((name, letters(m1[p]), letters(m2[p]), chr(33 + q)))
            if q != 20 + 10 * (copies - 1):
                marked.add(name.encode())
    for s in range(singles):
        name = "single%d" % s
        entries.append((name, letters(m1[s]), letters(rng.integers(0, 4, 100)), chr(33 + 60)))
        marked.add(name.encode())
    order = rng.permutation(len(entries))
    paths = [str(tmp / ("planted%d_%d.fq" % (pairs, i))) for i in (1, 2)]
    for i, path in enumerate(paths):
        with open(path, "w") as o:
            for e in order:
                name, a, b, q = entries[e]
                o.write("@%s/%d\n%s\n+\n%s\n" % (name, i + 1, (a, b)[i], q * 100))
    return S, paths, marked, len(entries)


def decode(path):
    """FILE -> (the header's bytes, the unframed records, their list)"""
    head, body = B.skip_header(gzip.decompress(open(path, "rb").read()))
    return head, body, B.split_records(body)


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


def flag_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def test_planted_copies_are_marked_and_nothing_else(tmp_path):
    import kiss_amd.bam_writer as W
    from tests.test_fm_insert_gpu import truth_index
    from tests.test_map_file_gpu import LIBRARY
    S, paths, marked, count = planted_files(tmp_path, 20, 10)
    assert len(marked) == 40 + 10 and count == 70
    f = truth_index(S)
    try:
        records = dict(bounds=[0, S.size // 3, S.size], ref_names=["one", "two"])
        out = str(tmp_path / "marked.bam")
        b = W.write_bam(out, f, paths[0], S, paths[1], batch_reads=16, version="X", sort=True, markdup=True, bai=True, **LIBRARY, **records)
        _, _, recs = decode(out)
        assert len(recs) == b["records"] >= 2 * count
        got = {name_of(r) for r in recs if flag_of(r) & 0x400}
        assert got == marked
        assert all(bool(flag_of(r) & 0x400) == (name_of(r) in marked) for r in recs)  # every record of such a template, and no other
        rep = b["markdup_report"]
        assert (rep["dup_pairs"], rep["dup_fragments"], rep["templates"], rep["pairs"], rep["fragments"]) == (40, 10, 70, 60, 10)
        assert rep["dup_records"] == sum(1 for r in recs if flag_of(r) & 0x400) >= 100
    finally:
        f.close()


def test_write_bam_marks_the_whole_file_however_it_is_cut(tmp_path):
    import kiss_amd.bam_writer as W
    from kiss_amd.batches import map_file
    from tests.test_fm_insert_gpu import truth_index
    from tests.test_map_file_gpu import LIBRARY
    S, paths, marked, count = planted_files(tmp_path, 3, 2)
    assert count == 11 and len(marked) == 8
    f = truth_index(S)
    try:
        records = dict(bounds=[0, S.size // 3, S.size], ref_names=["one", "two"])
        at = lambda k: str(tmp_path / k)  # noqa: E731
        kw = dict(version="X", sort=True, bai=True, **LIBRARY, **records)
        for compress in (False, True):
            a = W.write_bam(at("plain.bam"), f, paths[0], S, paths[1], batch_reads=7, compress=compress, **kw)
            assert "markdup_report" not in a
            head, plain, plain_recs = decode(at("plain.bam"))
            plain_bai = open(at("plain.bam.bai"), "rb").read()
            assert not any(flag_of(r) & 0x400 for r in plain_recs)
            seen = set()
            for batch_reads in (1, 7, count, count + 1):
                b = W.write_bam(at("marked.bam"), f, paths[0], S, paths[1], batch_reads=batch_reads, compress=compress, markdup=True, **kw)
                blob = open(at("marked.bam"), "rb").read()
                got_head, got, recs = decode(at("marked.bam"))
                assert got_head == head and len(got) == len(plain) and b["records"] == a["records"] == len(recs)
                assert b.keys() - a.keys() == {"markdup_report"} and b["batches"] == -(-count // batch_reads)
                # the unmarked file with bit 0x400 set where a planted name stands: nothing but bytes 18 - 19 of records differs
                want = b"".join(r[:18] + struct.pack("<H", flag_of(r) | (0x400 if name_of(r) in marked else 0)) + r[20:] for r in plain_recs)
                assert got == want, (compress, batch_reads)
                assert sum(1 for r in recs if flag_of(r) & 0x400) == b["markdup_report"]["dup_records"] >= 16
                assert open(at("marked.bam.bai"), "rb").read() == plain_bai
                seen.add(blob)
            assert len(seen) == 1  # byte-identical across the batch sizes
            low = W.write_bam(at("low.bam"), f, paths[0], S, paths[1], batch_reads=7, compress=compress, markdup=dict(min_qual=41), **kw)
            # no quality of a pair reaches 41: every score is 0 and the first copy in the file stays, whichever it is
            assert (low["markdup_report"]["dup_pairs"], low["markdup_report"]["dup_fragments"]) == (6, 2)
            assert len(decode(at("low.bam"))[1]) == len(got)
        with pytest.raises(ValueError, match="write_bam"):
            list(map_file(f, paths[0], S, paths[1], batch_reads=7, bam=True, bam_markdup=True, **LIBRARY, **records))
        for how in (dict(), dict(compress=True), dict(sort=False)):
            with pytest.raises(ValueError, match="sort=True"):
                W.write_bam(at("never.bam"), f, paths[0], S, paths[1], batch_reads=7, version="X", markdup=True, **how, **LIBRARY, **records)
        import os
        assert not os.path.exists(at("never.bam"))
    finally:
        f.close()
