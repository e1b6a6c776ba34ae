"""`kiss fmindex_query ... --sam --bam FILE --bam-sort --bam-markdup` on the inputs of tests/test_cli_bam_gpu.py with planted copies
(every read file behind itself: the second copy of every mapped read or pair is a duplicate).  The file decodes to the records of the
run without the option with FLAG 0x400 set exactly where tests/markdup_model.py sets it on the records as they were written, and to
the records of kiss_amd.bam_writer.write_bam(sort=True, markdup=True) on the same files; stdout and FILE.bai are byte for byte those
of the run without the option; with --bam-compress and --bam-index; the option is refused without --bam-sort; `kiss -h` does not
mention it and `kiss --help-bam` does.  Single end, paired, with --rescue --md, FASTQ, and in batches of three."""
import gzip
import os

import pytest

from tests import bam_model as B
from tests import bam_sort_model as SM
from tests import gen
from tests import markdup_model as M
from tests.test_cli_bam_gpu import VARIANTS, inputs, kiss  # noqa: F401
from tests.test_cli_sam_gpu import RECORDS

pytestmark = pytest.mark.gpu

# what write_bam takes for the options of a variant
PYTHON = {
    "single": dict(both_strands=True),
    "paired": dict(),
    "rescue, md": dict(rescue=True, want_md=True),
    "fastq": dict(both_strands=True, want_md=True),
    "batches of 3": dict(batch_reads=3, insert="auto"),
}


@pytest.fixture(scope="module")
def planted(inputs):  # noqa: F811
    """the inputs with every read file written twice into one file"""
    def twice(path):
        to = path + ".twice"
        if not os.path.exists(to):
            body = open(path).read()
            with open(to, "w") as o:
                o.write(body + body)
        return to
    return dict(inputs, reads=twice(inputs["reads"]), at=lambda name: twice(inputs["at"](name)))


@pytest.fixture(scope="module")
def index():
    import kiss_amd
    import kiss_amd.fm_index as fm
    S = gen.iid(sum(r[2] for r in RECORDS), 41)  # (the text of tests/test_cli_sam_gpu.make_inputs)
    with kiss_amd.Context(max_n=1 << 20) as ctx:
        sa = ctx.suffix_sort(S, kiss_amd.K_UNBOUNDED)
    f = fm.FMIndex(sa_intv=4).build(S, sa=sa, exact_sa=True)
    yield f, S
    f.close()


def records_of(path):
    head, body = B.skip_header(gzip.decompress(open(path, "rb").read()))
    return head, B.split_records(body)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_bam_markdup_on_the_command_line(planted, index, variant):
    import kiss_amd.bam_writer as W
    options = VARIANTS[variant](planted)
    common = ["fmindex_query", planted["fa"]] + options + ["--chain", "--align", "--sam"]
    at = lambda k: os.path.join(planted["tmp"], k)  # noqa: E731
    names = [name.encode() for name, _, _ in RECORDS]
    r = kiss(*common, "--bam", at("written.bam"))
    assert r.returncode == 0, r.stderr
    head, written = records_of(at("written.bam"))
    version = head[8:8 + int.from_bytes(head[4:8], "little")].rsplit(b"VN:", 1)[1].strip().decode()
    # the model: the records as they were written, marked, then sorted
    marked = M.markdup_model(*M.join(written), len(names))
    rep = marked["report"]
    assert len(written) >= 16 and rep["dup_records"] >= 6 and rep["dup_pairs"] + rep["dup_fragments"] >= 4
    want = SM.sort(*SM.pack(B.split_records(marked["bam"].tobytes())), len(names))
    want_records = B.split_records(want["bam"].tobytes())
    for more in ([], ["--bam-compress"]):
        for p in (at("sorted.bam"), at("sorted.bam.bai"), at("marked.bam"), at("marked.bam.bai")):
            if os.path.exists(p):
                os.remove(p)
        plain = kiss(*common, "--bam", at("sorted.bam"), "--bam-sort", "--bam-index", *more)
        assert plain.returncode == 0 and b"bam markdup" not in plain.stderr, plain.stderr
        r = kiss(*common, "--bam", at("marked.bam"), "--bam-sort", "--bam-markdup", "--bam-index", *more)
        assert r.returncode == 0, r.stderr
        assert r.stdout == plain.stdout == b""
        line = b"[info] bam markdup: templates: %d, duplicate pairs: %d, duplicate fragments: %d, duplicate records: %d\n" % (
            rep["templates"], rep["dup_pairs"], rep["dup_fragments"], rep["dup_records"])
        assert line in r.stderr and r.stderr.index(line) < r.stderr.index(b"[info] bam sort:")
        blob = open(at("marked.bam"), "rb").read()
        assert blob.endswith(B.BGZF_EOF)
        got_head, got = records_of(at("marked.bam"))
        plain_head, unmarked = records_of(at("sorted.bam"))
        assert got_head == plain_head and b"SO:coordinate" in got_head
        assert got == want_records, (variant, more)
        # the run without the option, and what the option changed in it: bit 0x400 of records, nothing else
        assert [x[:18] + bytes([x[18], x[19] & ~4 & 0xFF]) + x[20:] for x in got] == unmarked
        assert not any(x[19] & 4 for x in unmarked) and sum(1 for x in got if x[19] & 4) == rep["dup_records"]
        assert [B.bam_to_sam(x, names).split(b"\t", 2)[2] for x in got] == [B.bam_to_sam(x, names).split(b"\t", 2)[2] for x in unmarked]
        assert open(at("marked.bam.bai"), "rb").read() == open(at("sorted.bam.bai"), "rb").read()
        if not more:
            assert len(blob) == os.path.getsize(at("sorted.bam"))  # (stored blocks: not a byte more)
    # --bam-markdup-min-qual: above every quality nothing counts, and the first of every group stays
    r = kiss(*common, "--bam", at("marked.bam"), "--bam-sort", "--bam-markdup", "--bam-markdup-min-qual", "200")
    assert r.returncode == 0, r.stderr
    flat = M.markdup_model(*M.join(written), len(names), 200)
    assert records_of(at("marked.bam"))[1] == B.split_records(SM.sort(*SM.pack(B.split_records(flat["bam"].tobytes())), len(names))["bam"].tobytes())
    # the same files through write_bam
    f, S = index
    files = [options[options.index(k) + 1] if k in options else None for k in ("--seeds", "--mates")]
    b = W.write_bam(at("python.bam"), f, files[0], S, files[1], ref_names=[name for name, _, _ in RECORDS], bounds=planted["bounds"],
                    version=version, sort=True, markdup=True, **PYTHON[variant])
    py_head, py = records_of(at("python.bam"))
    assert py_head == got_head and py == want_records, variant
    assert {k: b["markdup_report"][k] for k in rep} == rep


def test_bam_markdup_goes_with_a_sorted_file_and_is_in_the_bam_help_only(planted):
    no = os.path.join(planted["tmp"], "no.bam")
    common = ["fmindex_query", planted["fa"], "--seeds", planted["reads"], "--both-strands", "--chain", "--align", "--sam"]
    r = kiss(*common, "--bam", no, "--bam-markdup")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-markdup goes with --bam-sort" in r.stderr and not os.path.exists(no)
    r = kiss(*common, "--bam-markdup")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-markdup goes with --bam-sort" in r.stderr
    r = kiss(*common, "--bam", no, "--bam-sort", "--bam-markdup-min-qual", "3")
    assert r.returncode != 0 and r.stdout == b"" and b"--bam-markdup-min-qual goes with --bam-markdup" in r.stderr and not os.path.exists(no)
    h = kiss("--help-bam")
    assert b"--bam-markdup" in h.stderr and b"kiss_hip_bam_markdup_host" in h.stderr and b"--bam-markdup-min-qual Q" in h.stderr
    assert b"--bam-markdup" not in kiss("-h").stderr
