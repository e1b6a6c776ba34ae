"""FMIndex.map(pileup=...), map_pairs(pileup=...) and kiss_amd.batches.map_file(pileup=...): the planes, counted on the device from
the buffers the stages left there, (a) against tests/fm_pileup_model.py applied to the RETURNED records, (b) against the truth on
reads cut from a random text -- coverage, a planted substitution, a planted deletion --, (c) summed over the batches of a file
against one call on the whole file.  Without pileup every result is what it was."""
import numpy as np
import pytest

from tests import fm_pileup_model as pm
from tests.test_fm_mm_gpu import TEXTS, text

pytestmark = pytest.mark.gpu
PILEUP_KEYS = {"pileup", "pileup_report"}


def same_as_model(res, S, reads, both, paired=False, lo=0, hi=None, counts=None, **params):
    want = pm.pileup(S, reads, res["alignments"], res["chain_index"], res["cigar"], res["cigar_index"], both, hits=res["hits"],
                     pairs=res["pairs"] if paired else None, lo=lo, hi=hi, counts=counts, **params)
    got = res["pileup"]
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32 and got.shape == want["counts"].shape
    assert np.array_equal(got, want["counts"]), np.argwhere(got != want["counts"])[:5]
    for k in pm.COUNTS:
        assert res["pileup_report"][k] == want[k], k
    assert want["bad"] == 0
    return want


def same_without_pileup(res, plain):
    from tests.test_fm_md_gpu import same_results
    assert PILEUP_KEYS <= res.keys() and not PILEUP_KEYS & plain.keys()
    same_results({k: v for k, v in res.items() if k not in PILEUP_KEYS}, plain)


# ---- against the model -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("both", (False, True))
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_map_with_pileup_equals_the_model_on_the_returned_records(name, both):
    import torch
    from tests.test_fm_align_gpu import reads_of
    from tests.test_fm_chain_gpu import index_of
    assert len(TEXTS) == 7
    f, S, reads = index_of(name, 4), text(name), reads_of(name)
    n = S.size
    common = dict(both_strands=both, chain_params=dict(min_score=25, band=100))
    plain = f.map(reads, S, 15, 0, 200, **common)
    res = f.map(reads, S, 15, 0, 200, pileup=True, **common)
    same_without_pileup(res, plain)
    want = same_as_model(res, S, reads, both)
    assert want["items"] == res["hits"].size and want["filtered"] == int((res["hits"]["flags"] & 2 != 0).sum())
    if name in ("genome", "iid"):
        assert want["counted"] >= 4 and want["columns"] > 300 and want["alt_columns"] > 0 and res["pileup"][pm.COV].max() >= 1
    # a window and a filter; an array and a tensor to add to
    lo, hi = n // 4, n - n // 3
    start = np.random.default_rng(1).integers(0, 9, (8, hi - lo)).astype(np.uint32)
    res = f.map(reads, S, 15, 0, 200, pileup=dict(lo=lo, hi=hi, counts=start, min_mapq=1, skip_flags=0), **common)
    same_as_model(res, S, reads, both, lo=lo, hi=hi, counts=start, min_mapq=1, skip_flags=0)
    tensor = torch.from_numpy(start.view(np.int32)).to("cuda:0")
    res = f.map(reads, S, 15, 0, 200, pileup=dict(lo=lo, hi=hi, counts=tensor), **common)
    assert res["pileup"] is tensor
    res["pileup"] = tensor.cpu().numpy().view(np.uint32)
    same_as_model(res, S, reads, both, lo=lo, hi=hi, counts=start)
    with pytest.raises(ValueError):
        f.map(reads, S, pileup=True, want_cigar=False)
    with pytest.raises(TypeError):
        f.map(reads, S, pileup=dict(min_mapqq=3))
    with pytest.raises(ValueError):
        f.map(reads, S, pileup=dict(lo=n + 1))


@pytest.mark.parametrize("rescue", (None, True))
@pytest.mark.parametrize("name", ("genome", "iid", "periodic", "n5"))
def test_map_pairs_with_pileup_with_and_without_rescue(name, rescue):
    from tests.test_fm_chain_gpu import index_of
    from tests.test_fm_pair_gpu import mates_of
    f, S = index_of(name, 4), text(name)
    m1, m2 = mates_of(name)
    reads = [r for pr in zip(m1, m2) for r in pr]
    common = dict(chain_params=dict(min_score=25, band=100), select_params=dict(min_score=20), ins_max=400, rescue=rescue)
    plain = f.map_pairs(m1, m2, S, 15, 0, 200, **common)
    res = f.map_pairs(m1, m2, S, 15, 0, 200, pileup=True, **common)
    same_without_pileup(res, plain)
    want = same_as_model(res, S, reads, True, paired=True)
    assert want["items"] == 2 * len(m1) and want["unmapped"] == int((res["pairs"]["hit1"] == 0xFFFFFFFF).sum() + (res["pairs"]["hit2"] == 0xFFFFFFFF).sum())
    res = f.map_pairs(m1, m2, S, 15, 0, 200, pileup=dict(proper_only=1, min_mapq=3), **common)
    want = same_as_model(res, S, reads, True, paired=True, proper_only=1, min_mapq=3)
    if name in ("genome", "iid"):
        assert want["filtered"] > 0 and want["counted"] > 0


# ---- against the truth -------------------------------------------------------------------------------------------------------------
def revcomp(r):
    return (3 - r[::-1]).astype(np.uint8)


def truth_case():
    """a random text of 20 000 bases and the loci of 400 reads of 100 bases: 30 that cover position p with it 20 .. 79 bases into
    the read, 20 that cover d .. d + 2 with them 30 .. 70 bases in, 350 that touch neither; d is a place where a deletion of three
    bases can be written in one way only"""
    rng = np.random.default_rng(2024)
    S = rng.integers(0, 4, 20_000, dtype=np.uint8)
    p = 10_000
    d = next(x for x in range(15_000, 15_100) if S[x - 1] != S[x + 2] and S[x] != S[x + 3])
    over_p = (p - 20 - rng.choice(60, 30, replace=False)).tolist()
    over_d = (d - 30 - rng.choice(41, 20, replace=False)).tolist()
    free = [a for a in rng.permutation(S.size - 100).tolist() if not (p - 99 <= a <= p) and not (d - 103 <= a <= d + 2)][:350]
    return S, p, d, over_p, over_d, free


def mapped_as_planted(res, loci, ops_of):
    """the precondition, for every read: its primary hit lies at its locus with the ops that were planted"""
    for q, a in enumerate(loci):
        h0, h1 = int(res["hit_index"][q]), int(res["hit_index"][q + 1])
        assert h1 > h0, "read %d has no hit" % q
        hit = res["hits"][h0]
        aln = int(hit["aln"])
        rec = res["alignments"][aln]
        ops = [(int(w) & 15, int(w) >> 4) for w in res["cigar"][int(res["cigar_index"][aln]):int(res["cigar_index"][aln + 1])]]
        assert not hit["flags"] & 2 and int(rec["tbeg"]) == a and ops == ops_of(q, a), (q, a, int(rec["tbeg"]), ops)
        assert bool(hit["flags"] & 1) == bool(q % 2)


def test_against_the_truth_coverage_a_substitution_and_a_deletion():
    from tests.test_fm_insert_gpu import truth_index
    S, p, d, over_p, over_d, free = truth_case()
    loci = over_p + over_d + free
    assert len(loci) == 400 and sum(a <= p < a + 100 for a in loci) == 30
    strand = lambda q, r: revcomp(r) if q % 2 else r  # noqa: E731 (every second read comes from the other strand)
    f = truth_index(S)
    try:
        # 1. without errors: COV is the coverage of the true loci, every other plane is zero
        reads = [strand(q, S[a:a + 100].copy()) for q, a in enumerate(loci)]
        res = f.map(reads, S, both_strands=True, pileup=True)
        mapped_as_planted(res, loci, lambda q, a: [(0, 100)])
        cover = np.zeros(S.size + 1, np.int64)
        np.add.at(cover, loci, 1)
        np.add.at(cover, [a + 100 for a in loci], -1)
        cover = np.cumsum(cover)[:-1]
        assert np.array_equal(res["pileup"][pm.COV], cover) and not res["pileup"][1:].any()
        assert res["pileup_report"]["columns"] == 40_000 and res["pileup_report"]["counted"] == 400
        # 2. a substitution at p in the 30 reads that cover it
        planted = (int(S[p]) + 2) & 3
        reads = []
        for q, a in enumerate(loci):
            r = S[a:a + 100].copy()
            if a <= p < a + 100:
                r[p - a] = planted
            reads.append(strand(q, r))
        res = f.map(reads, S, both_strands=True, pileup=True)
        mapped_as_planted(res, loci, lambda q, a: [(0, 100)])
        alt = np.zeros((5, S.size), np.int64)
        alt[planted, p] = 30
        assert np.array_equal(res["pileup"][pm.COV], cover) and np.array_equal(res["pileup"][pm.ALT_A:pm.ALT_N + 1], alt)
        assert not res["pileup"][pm.DEL:].any() and res["pileup_report"]["alt_columns"] == 30
        # 3. the three bases d .. d + 2 missing from the 20 reads that cover them
        reads = [strand(q, np.concatenate([S[a:d], S[d + 3:a + 103]]) if a in over_d else S[a:a + 100].copy()) for q, a in enumerate(loci)]
        res = f.map(reads, S, both_strands=True, pileup=True)
        mapped_as_planted(res, loci, lambda q, a: [(0, d - a), (2, 3), (0, 100 - (d - a))] if a in over_d else [(0, 100)])
        dele = np.zeros(S.size, np.int64)
        dele[d:d + 3] = 20
        cov = np.zeros(S.size, np.int64)
        for a in loci:
            if a in over_d:
                cov[a:d] += 1
                cov[d + 3:a + 103] += 1
            else:
                cov[a:a + 100] += 1
        assert np.array_equal(res["pileup"][pm.DEL], dele) and np.array_equal(res["pileup"][pm.COV], cov)
        assert not res["pileup"][pm.ALT_A:pm.ALT_N + 1].any() and not res["pileup"][pm.INS].any()
        assert res["pileup_report"]["deleted_bases"] == 60
    finally:
        f.close()


# ---- over the batches of a file ----------------------------------------------------------------------------------------------------
def test_map_file_sums_the_batches_into_one_tensor(tmp_path_factory):
    import torch
    from kiss_amd.batches import map_file
    from tests.test_fm_insert_gpu import insert_truth_case, truth_index
    from tests.test_map_file_gpu import LIBRARY, write_fastq
    S, m1, m2, _ = insert_truth_case(200, 10)
    pick = list(range(8)) + list(range(200, 202))
    s1, s2 = [m1[p] for p in pick], [m2[p] for p in pick]
    tmp = tmp_path_factory.mktemp("map_pileup")
    paths = {k: str(tmp / k) for k in ("s1.fq", "s2.fq", "single.fq")}
    write_fastq(paths["s1.fq"], s1, "/1", 1)
    write_fastq(paths["s2.fq"], s2, "/2", 2)
    single = [r for pair in zip(s1, s2) for r in pair]
    write_fastq(paths["single.fq"], single, "", 3)
    f = truth_index(S)
    try:
        Q, P = len(single), len(s1)
        whole = f.map(single, S, both_strands=True, pileup=True)
        assert whole["pileup_report"]["counted"] >= 16 and whole["pileup"][pm.COV].sum() == whole["pileup_report"]["columns"]
        for batch_reads in (1, 7, Q, Q + 1):
            got = list(map_file(f, paths["single.fq"], S, batch_reads=batch_reads, both_strands=True, pileup=True))
            assert len(got) == -(-Q // batch_reads)
            last = got[-1]
            assert isinstance(last["pileup"], torch.Tensor) and all(x["pileup"] is last["pileup"] for x in got)  # one tensor, allocated once
            assert np.array_equal(last["pileup"].cpu().numpy().view(np.uint32), whole["pileup"]), batch_reads
            for k in pm.COUNTS:
                assert last["pileup_report"][k] == whole["pileup_report"][k], (batch_reads, k)
        # paired, with the rescue, a filter and a window, onto a tensor of the caller's
        lo, hi = 100, S.size - 50
        opts = dict(proper_only=1, min_mapq=1, lo=lo, hi=hi)
        pw = f.map_pairs(s1, s2, S, rescue=True, pileup=opts, **LIBRARY)
        assert pw["pileup_report"]["counted"] >= 12
        for batch_reads in (3, P + 1):
            mine = torch.full((8, hi - lo), 5, dtype=torch.int32, device="cuda:0")
            got = list(map_file(f, paths["s1.fq"], S, paths["s2.fq"], batch_reads=batch_reads, rescue=True, pileup=dict(opts, counts=mine), **LIBRARY))
            assert got[-1]["pileup"] is mine and np.array_equal(mine.cpu().numpy().view(np.uint32), pw["pileup"] + np.uint32(5))
            for k in pm.COUNTS:
                assert got[-1]["pileup_report"][k] == pw["pileup_report"][k], (batch_reads, k)
        plain = list(map_file(f, paths["single.fq"], S, batch_reads=7, both_strands=True))
        assert not any(PILEUP_KEYS & x.keys() for x in plain)
    finally:
        f.close()
