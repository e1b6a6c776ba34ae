"""FMIndex.map(sam=True), map_pairs(sam=True) and kiss_amd.batches.map_file(sam=True): the lines, written on the device from the
buffers the stages left there, against tests/fm_sam_model.py on a batch rebuilt from the RETURNED arrays; without sam every
result is what it was; the lines of a file mapped in batches are the lines of the whole file; the default names."""
import numpy as np
import pytest

from tests import fm_sam_model as M
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu

SAM_KEYS = {"sam", "sam_line_index", "sam_read_line", "sam_report"}
REPORT = ("lines", "sam_bytes", "unmapped_lines", "longest", "bad", "first_bad")
REF_NAMES = ["chrA", "chrB"]


def rows(records, width):
    return np.array(records.tolist(), np.int64).reshape(-1, width)


def batch_of(res, reads, names, qual, ref_names, bounds):
    """the model's batch from what a map call returned"""
    index = np.zeros(len(reads) + 1, np.uint64)
    np.cumsum([len(r) for r in reads], out=index[1:])
    return {"reads": np.concatenate(reads).astype(np.uint8), "read_index": index, "qual": None if qual is None else np.concatenate(qual),
            "names": [x if isinstance(x, bytes) else x.encode() for x in names], "alns": rows(res["alignments"], 12), "cigar": res["cigar"],
            "cigar_index": res["cigar_index"], "hits": rows(res["hits"], 8), "hit_index": res["hit_index"],
            "pairs": rows(res["pairs"], 10) if "pairs" in res else None, "source": res.get("aln_source"),
            "first_alns": res["first_pass"]["alignments"] if "first_pass" in res else 0, "md": res.get("md"), "md_index": res.get("md_index"),
            "ref_names": [x.encode() for x in (ref_names or [])], "bounds": np.asarray((bounds or [0, 0]) if ref_names else [0], np.uint64)}


def same_as_model(res, b):
    want = M.sam_model(b)
    assert isinstance(res["sam"], bytes) and res["sam"] == want["sam"]
    assert np.array_equal(res["sam_line_index"], want["line_index"]) and np.array_equal(res["sam_read_line"], want["read_line"])
    assert {k: res["sam_report"][k] for k in REPORT} == want["report"]
    return want


def same_without_sam(res, plain):
    from tests.test_fm_md_gpu import same_results
    assert SAM_KEYS <= res.keys() and not SAM_KEYS & plain.keys()
    same_results({k: v for k, v in res.items() if k not in SAM_KEYS}, plain)


def quals_of(reads, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(33, 127, len(r)).astype(np.uint8) for r in reads]


def parameter_sets(n):
    """without anything; with MD and the records: two where the text has two bases, else one (a text of no base takes no
    bounds: the one record is named alone)"""
    if n >= 2:
        return (dict(), dict(want_md=True, bounds=[0, n // 2, n], ref_names=REF_NAMES))
    return (dict(), dict(want_md=True, ref_names=REF_NAMES[:1], **(dict(bounds=[0, n]) if n else {})))


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_sam_equals_the_model(name):
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    assert len(TEXTS) == 7
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    qual = quals_of(reads, 5)
    names = ["read%d/x" % (q * q) for q in range(len(reads))]
    lines = 0
    for k, params in enumerate(parameter_sets(S.size)):
        common = dict(both_strands=True, chain_params=dict(min_score=25, band=100), **params)
        given = dict(names=names, qual=qual) if k else {}
        res = f.map(reads, S, 15, 0, 200, sam=True, **given, **common)
        plain = f.map(reads, S, 15, 0, 200, **{x: v for x, v in common.items() if x != "ref_names"})
        same_without_sam(res, plain)
        want = same_as_model(res, batch_of(res, reads, names if k else [str(q) for q in range(len(reads))], qual if k else None,
                                           params.get("ref_names"), params.get("bounds")))
        lines += want["report"]["lines"] - want["report"]["unmapped_lines"]
        assert (b"MD:Z:" in res["sam"]) == (k == 1 and res["hits"].size > 0)
    if name in ("genome", "iid"):
        assert lines >= 8
    with pytest.raises(ValueError):
        f.map(reads, S, sam=True, want_cigar=False)
    with pytest.raises(ValueError):
        f.map(reads, S, names=names)


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_pairs_with_sam_equals_the_model(name):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    m1, m2 = mates_of(name)
    reads = [r for pr in zip(m1, m2) for r in pr]
    P = len(m1)
    q1, q2 = quals_of(m1, 6), quals_of(m2, 7)
    names = ["pair:%d" % p for p in range(P)]
    for k, params in enumerate(parameter_sets(S.size)):
        common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=True if k else None, **params)
        given = dict(names=names, qual=(q1, q2)) if k else {}
        res = f.map_pairs(m1, m2, S, 15, 0, 200, sam=True, **given, **common)
        plain = f.map_pairs(m1, m2, S, 15, 0, 200, **{x: v for x, v in common.items() if x != "ref_names"})
        same_without_sam(res, plain)
        both = [n for n in (names if k else [str(p) for p in range(P)]) for _ in (0, 1)]
        b = batch_of(res, reads, both, [x for pr in zip(q1, q2) for x in pr] if k else None, params.get("ref_names"), params.get("bounds"))
        same_as_model(res, b)
        if k:
            rescued = b["source"] is not None and bool(np.any(b["source"][rows(res["hits"], 8)[:, 0]] >= b["first_alns"]))
            assert (b"YR:i:1" in res["sam"]) == rescued
    with pytest.raises(ValueError):
        f.map_pairs(m1, m2, S, sam=True, qual=(q1, q2[:-1]))


def test_map_file_with_sam_gives_the_lines_of_the_whole_file(tmp_path_factory):
    from kiss_amd.batches import map_file
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_sam")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq")}
    write_fastq(paths["s1.fq"], s1, "/1", 1)
    write_fastq(paths["s2.fq"], s2, "/2", 2)
    single = [r for pair in zip(s1, s2) for r in pair]
    write_fastq(paths["single.fq"], single, "", 3)
    f = truth_index(S)
    try:
        n, Q, P = S.size, len(single), len(s1)
        records = dict(bounds=[0, n // 3, n], ref_names=["one", "two"])
        # single end: the whole file is one batch of Q + 1 reads; it equals the model with the file's names and qualities
        whole = list(map_file(f, paths["single.fq"], S, batch_reads=Q + 1, both_strands=True, want_md=True, sam=True, **records))
        assert len(whole) == 1
        w = whole[0]
        names = [str(q) if q % 5 == 3 else "p%d" % q for q in range(Q)]
        assert w["names"] == names
        index = np.zeros(Q + 1, np.int64)
        np.cumsum([len(r) for r in single], out=index[1:])
        qual = [w["qual"][index[q]:index[q + 1]] for q in range(Q)]
        same_as_model(w, batch_of(w, single, names, qual, records["ref_names"], records["bounds"]))
        for batch_reads in (1, 7):
            got = list(map_file(f, paths["single.fq"], S, batch_reads=batch_reads, both_strands=True, want_md=True, sam=True, **records))
            assert len(got) == -(-Q // batch_reads) and b"".join(x["sam"] for x in got) == w["sam"]
        # paired: FASTQ mate names lose /1 and /2; a pair without a name gets its number in the file
        pw = list(map_file(f, paths["s1.fq"], S, paths["s2.fq"], batch_reads=P + 1, rescue=True, want_md=True, sam=True, **records, **LIBRARY))
        assert len(pw) == 1
        w = pw[0]
        pnames = [str(p) if p % 5 == 3 else "p%d" % p for p in range(P) for _ in (0, 1)]
        assert w["names"] == pnames
        both = [r for pair in zip(s1, s2) for r in pair]
        qual = [w["qual"][100 * q:100 * (q + 1)] for q in range(2 * P)]
        assert all(len(r) == 100 for r in both)
        same_as_model(w, batch_of(w, both, pnames, qual, records["ref_names"], records["bounds"]))
        for batch_reads in (1, 7):
            got = list(map_file(f, paths["s1.fq"], S, paths["s2.fq"], batch_reads=batch_reads, rescue=True, want_md=True, sam=True, **records,
                                **LIBRARY))
            assert len(got) == -(-P // batch_reads) and b"".join(x["sam"] for x in got) == w["sam"]
        plain = list(map_file(f, paths["s1.fq"], S, paths["s2.fq"], batch_reads=7, rescue=True, want_md=True, **LIBRARY))
        assert not any(SAM_KEYS & x.keys() for x in plain)
        with pytest.raises(ValueError):
            next(map_file(f, paths["single.fq"], S, sam=True, names=["a"]))
    finally:
        f.close()


def test_default_names():
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of("genome", 4), text("genome")
    m1, m2 = mates_of("genome")
    res = f.map(m1, S, both_strands=True, sam=True)
    first = [ln.split(b"\t")[0] for ln in res["sam"].split(b"\n")[:-1]]
    rl = res["sam_read_line"]
    assert [first[int(rl[q])] for q in range(len(m1))] == [str(q).encode() for q in range(len(m1))]
    assert all(first[k] == str(q).encode() for q in range(len(m1)) for k in range(int(rl[q]), int(rl[q + 1])))
    res = f.map_pairs(m1, m2, S, sam=True)
    first = [ln.split(b"\t")[0] for ln in res["sam"].split(b"\n")[:-1]]
    rl = res["sam_read_line"]
    assert all(first[k] == str(q // 2).encode() for q in range(2 * len(m1)) for k in range(int(rl[q]), int(rl[q + 1])))
    assert len(first) == int(rl[-1]) == res["sam_report"]["lines"]
