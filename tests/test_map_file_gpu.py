"""kiss_amd.batches.map_file against map / map_pairs on the whole file: every stage behind the parse
treats a read or a pair on its own, so read by read the hits, the alignments they name (with MAPQ, CIGAR and MD) and the pair
records are the same however the file is cut; indices are compared after rebasing.  The insert size is the exception: it is
estimated once, from batch 0.  The text and the library are those of tests/test_fm_insert_gpu.py (60 000 bases, fragments of
1400 .. 1600), 16 good pairs and 4 with a mate that has no seed."""
import numpy as np
import pytest

from kiss_amd.batches import map_file
from tests.test_fm_insert_gpu import insert_truth_case, truth_index

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
LIBRARY = dict(ins_min=1000, ins_max=2000, ins_mean=1500)


def write_fastq(path, reads, tag, seed):
    rng = np.random.default_rng(seed)
    with open(path, "w") as o:
        for q, r in enumerate(reads):
            qual = "".join(chr(c) for c in rng.integers(33, 127, len(r)))
            o.write("@%s\n%s\n+\n%s\n" % ("" if q % 5 == 3 else "p%d%s extra" % (q, tag), "".join("ACGT"[int(c)] for c in r), qual))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    S, m1, m2, truth = insert_truth_case(200, 10)
    tmp = tmp_path_factory.mktemp("map_file")
    pick = list(range(16)) + list(range(200, 204))  # 16 good pairs, 4 whose damaged mate only the rescue finds
    small1, small2 = [m1[p] for p in pick], [m2[p] for p in pick]
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq", "l1.fq", "l2.fq", "few1.fq", "few2.fq")}
    write_fastq(paths["s1.fq"], small1, "/1", 1)
    write_fastq(paths["s2.fq"], small2, "/2", 2)
    write_fastq(paths["single.fq"], [r for pair in zip(small1, small2) for r in pair], "", 3)
    write_fastq(paths["l1.fq"], m1[:200], "/1", 4)
    write_fastq(paths["l2.fq"], m2[:200], "/2", 5)
    write_fastq(paths["few1.fq"], m1[:60], "/1", 6)
    write_fastq(paths["few2.fq"], m2[:60], "/2", 7)
    f = truth_index(S)
    yield dict(S=S, m1=m1, m2=m2, small1=small1, small2=small2, paths=paths, f=f)
    f.close()


def per_read(res, want_md):
    """[per read: [per hit: everything a hit says, with the alignment it names in the place of its number]]"""
    from kiss_amd.fm_md import md_strings
    md = md_strings(res["md"], res["md_index"]) if want_md else None
    hidx, cidx = res["hit_index"], res["cigar_index"]
    out = []
    for q in range(hidx.size - 1):
        hits = []
        for h in range(int(hidx[q]), int(hidx[q + 1])):
            hit = res["hits"][h]
            a = int(hit["aln"])
            hits.append((tuple(int(hit[k]) for k in ("flags", "mapq", "score", "sub", "n_sec", "head", "ref")), res["alignments"][a].tolist(),
                         res["cigar"][int(cidx[a]):int(cidx[a + 1])].tolist(), md[h] if want_md else None))
        out.append(hits)
    return out


def per_pair(res):
    """[per pair: the record with hit1 / hit2 counted from the first hit of their reads]"""
    hidx, out = res["hit_index"], []
    for p, rec in enumerate(res["pairs"]):
        r = {k: int(rec[k]) for k in rec.dtype.names}
        for k, q in (("hit1", 2 * p), ("hit2", 2 * p + 1)):
            if r[k] != NONE:
                r[k] -= int(hidx[q])
        out.append(r)
    return out


def gathered(batches, paired, want_md, batch_reads):
    reads, pairs, names, first, count = [], [], [], [], 0
    for b in batches:
        first.append(b["first_read"])
        records = (b["hit_index"].size - 1) // (2 if paired else 1)
        assert 0 < records <= batch_reads and b["first_read"] == count  # (none is empty)
        count += records
        reads += per_read(b, want_md)
        names += b["names"]
        if paired:
            pairs += per_pair(b)
        assert b["qual"].size == 100 * (b["hit_index"].size - 1)  # (the quality bytes of the batch's reads)
    return reads, pairs, names, first


@pytest.mark.parametrize("chunk_bytes", [64, 4096])
def test_single_end_batches_equal_map_of_the_whole_file(case, chunk_bytes):
    f, S = case["f"], case["S"]
    reads = [r for pair in zip(case["small1"], case["small2"]) for r in pair]
    Q = len(reads)
    assert Q == 40
    whole = f.map(reads, S, both_strands=True, want_md=True)
    want = per_read(whole, True)
    assert sum(1 for hits in want if hits) >= 32
    for batch_reads in (1, 7, Q, Q + 1):
        got = list(map_file(f, case["paths"]["single.fq"], S, batch_reads=batch_reads, chunk_bytes=chunk_bytes, both_strands=True, want_md=True))
        reads_got, _, names, first = gathered(got, False, True, batch_reads)
        assert reads_got == want and first == list(range(0, Q, batch_reads))  # (a chunk of 64 bytes holds no record: it grows)
        assert names == [str(q) if q % 5 == 3 else "p%d" % q for q in range(Q)]  # (a read without a name: its number in the file)


@pytest.mark.parametrize("rescue", [None, True])
@pytest.mark.parametrize("chunk_bytes", [64, 4096])
def test_paired_batches_equal_map_pairs_of_the_whole_file(case, chunk_bytes, rescue):
    f, S = case["f"], case["S"]
    P = len(case["small1"])
    assert P == 20
    whole = f.map_pairs(case["small1"], case["small2"], S, rescue=rescue, want_md=True, **LIBRARY)
    want_reads, want_pairs = per_read(whole, True), per_pair(whole)
    proper = whole["pair_report"]["proper"]
    assert proper > 16 if rescue else proper == 16  # (the rescue has something to do)
    for batch_reads in (1, 7, P, P + 1):
        got = list(map_file(f, case["paths"]["s1.fq"], S, case["paths"]["s2.fq"], batch_reads=batch_reads, chunk_bytes=chunk_bytes,
                            rescue=rescue, want_md=True, **LIBRARY))
        reads_got, pairs_got, names, first = gathered(got, True, True, batch_reads)
        assert reads_got == want_reads and pairs_got == want_pairs and first == list(range(0, P, batch_reads))
        assert names == [str(p) if p % 5 == 3 else "p%d" % p for p in range(P) for _ in (1, 2)]  # (/1 and /2 are stripped)


def test_the_insert_size_is_estimated_once_from_batch_0(case):
    f, S = case["f"], case["S"]
    got = list(map_file(f, case["paths"]["l1.fq"], S, case["paths"]["l2.fq"], batch_reads=100, insert="auto"))
    assert len(got) == 2 and [b["first_read"] for b in got] == [0, 100]
    first, second = got[0]["insert"], got[1]["insert"]
    assert first["applied"] and first["from_batch"] == 0 and first["report"]["samples"] == 100 and int(first["hist"].sum()) == 100
    assert first["ins_min"] <= 1400 and first["ins_max"] >= 1600
    assert second == {k: first[k] for k in ("applied", "ins_min", "ins_max", "ins_mean", "from_batch")}  # no report, no histogram
    assert all(b["pair_report"]["proper"] == 100 for b in got)
    # the second batch is what map_pairs makes of its pairs with batch 0's three values
    want = f.map_pairs(case["m1"][100:200], case["m2"][100:200], S, ins_min=first["ins_min"], ins_max=first["ins_max"], ins_mean=first["ins_mean"])
    assert per_pair(got[1]) == per_pair(want)
    # a first batch below min_samples: the defaults serve the whole file, and no pair of this library is proper under them
    got = list(map_file(f, case["paths"]["few1.fq"], S, case["paths"]["few2.fq"], batch_reads=20, chunk_bytes=1 << 16, insert="auto"))
    assert len(got) == 3
    assert got[0]["insert"]["applied"] is False and got[0]["insert"]["report"]["samples"] == 20
    for b in got:
        assert {k: b["insert"][k] for k in ("applied", "ins_min", "ins_max", "ins_mean", "from_batch")} == dict(
            applied=False, ins_min=0, ins_max=1000, ins_mean=400, from_batch=0)
        assert b["pair_report"]["proper"] == 0


def test_mate_files_of_different_lengths_and_bad_records(case, tmp_path):
    f, S = case["f"], case["S"]
    with pytest.raises(ValueError, match=r"s1\.fq runs out after 20 reads"):  # (the shorter file and its length)
        list(map_file(f, case["paths"]["s1.fq"], S, case["paths"]["few2.fq"], batch_reads=7, chunk_bytes=4096))
    with pytest.raises(ValueError, match=r"s2\.fq runs out after 20 reads"):
        list(map_file(f, case["paths"]["few1.fq"], S, case["paths"]["s2.fq"], batch_reads=20, chunk_bytes=4096))
    with pytest.raises(TypeError):
        next(map_file(f, case["paths"]["s1.fq"], S, case["paths"]["s2.fq"], overlap=3))
    lines = open(case["paths"]["single.fq"]).read().split("\n")
    lines[4 * 17 + 2] = "-"  # record 17 is bad: with batches of 7 the third batch meets it, and names it by its number in the file
    bad = tmp_path / "bad.fq"
    bad.write_text("\n".join(lines))
    batches = map_file(f, str(bad), S, batch_reads=7, chunk_bytes=4096, both_strands=True)
    assert [b["first_read"] for b in (next(batches), next(batches))] == [0, 7]
    with pytest.raises(ValueError, match="record 17"):
        next(batches)
