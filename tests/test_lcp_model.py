"""CPU side of the LCP array: the host models, the report struct's ABI, the C++ facade, and the CLI's refusal of
--output-lcp with a bounded k (decided before any device work)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import gen, lcp_model
from tests.test_abi import _sizeof_from_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _texts():
    rng = np.random.default_rng(3)
    out = [np.zeros(0, np.uint8), np.zeros(1, np.uint8), np.array([2, 1], np.uint8), np.zeros(40, np.uint8),
           np.tile(np.array([0, 1], np.uint8), 30), gen.periodic(200, 7, 1, 3), np.frombuffer(b"mississippi", np.uint8)]
    for _ in range(40):
        n = int(rng.integers(0, 120))
        out.append(rng.integers(0, int(rng.choice([1, 2, 4, 256])), n, dtype=np.uint8))
    return out


def test_kasai_matches_brute_force():
    for S in _texts():
        SA = lcp_model.naive_sa(S)
        assert np.array_equal(lcp_model.kasai(S, SA), lcp_model.brute(S, SA)), S


def test_hash_check_accepts_correct_and_rejects_wrong():
    for S in _texts():
        SA = lcp_model.naive_sa(S)
        LCP = lcp_model.kasai(S, SA)
        assert lcp_model.lcp_hash_check(S, SA, LCP)
        if S.size < 2:
            continue
        i = 1 + int(np.argmax(LCP[1:]))  # one entry too long, one too short
        for delta in (1, -1):
            if int(LCP[i]) + delta < 0:
                continue
            bad = LCP.astype(np.int64)
            bad[i] += delta
            with pytest.raises(AssertionError):
                lcp_model.lcp_hash_check(S, SA, bad)


def test_hash_check_on_long_lcps_in_chunks():
    # a periodic text with a unique last symbol: lcps of thousands of symbols, checked over several chunks
    S = gen.periodic(3000, 5, 2)
    S[S == 3] = 2
    S = np.concatenate([S, np.array([3], np.uint8)])
    SA = lcp_model.naive_sa(S)
    LCP = lcp_model.kasai(S, SA)
    assert int(LCP.max()) > 2000
    assert lcp_model.lcp_hash_check(S, SA, LCP, chunk=256)
    for i in (5, S.size - 1):
        bad = LCP.copy()
        bad[i] ^= 1
        with pytest.raises(AssertionError):
            lcp_model.lcp_hash_check(S, SA, bad, chunk=256)


def test_lcp_report_struct_matches_the_header():
    from kiss_amd import _lib
    assert ctypes.sizeof(_lib.LcpReport) == _sizeof_from_header("kiss_hip_lcp_report") == 64
    assert _lib.LcpReport.ms_scan_gather.offset == 56


def test_lcp_symbols_are_exported():
    import kiss_amd
    lib = kiss_amd.load()
    for s in ("kiss_hip_ctx_lcp_dna_u32_dev", "kiss_hip_ctx_lcp_u8_dev", "kiss_hip_lcp_dna_u32", "kiss_hip_lcp_u8"):
        assert hasattr(lib, s) and s in kiss_amd._lib.EXPORTED_SYMBOLS
    assert callable(kiss_amd.lcp_array) and callable(kiss_amd.lcp_array_bytes)


def test_cpp_facade_lcp_members_compile_and_link(tmp_path):
    src = tmp_path / "f.cpp"
    src.write_text('#include "kiss_amd/csrc/host/kiss_hip_sorter.hpp"\n'
                   "#include <string>\n"
                   "int main(int argc, char **) {\n"
                   "  if (argc < 2) return 0;\n"
                   "  std::vector<std::uint8_t> S{0, 1, 2, 3, 0, 1};\n"
                   "  auto SA = biovoltron::KissHipSorter<>::get_suffix_array_dna(S, 0xFFFFFFFFu);\n"
                   "  auto L = biovoltron::KissHipSorter<>::get_lcp_array_dna(S, SA);\n"
                   "  std::string t = \"banana\";\n"
                   "  auto L2 = biovoltron::KissHipSorter<std::uint64_t>::get_lcp_array(t, {});\n"
                   "  return (int)(L.size() + L2.size());\n}\n")
    exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-I", ROOT, str(src), "-o", str(exe),
                           "-L" + os.path.join(ROOT, "kiss_amd"), "-lkiss_hip", "-Wl,-rpath," + os.path.join(ROOT, "kiss_amd")])
    assert subprocess.call([str(exe)]) == 0


def test_cli_refuses_output_lcp_with_a_bounded_k(tmp_path):
    kiss = os.path.join(ROOT, "kiss_amd", "kiss")
    fa = tmp_path / "x.fa"
    fa.write_text(">chr1 test\nACGTACGTAAAACCCGGGTTT\n>chr2\nACGTNNACGT\n")  # 31 bases, 49 bytes
    lcp = tmp_path / "lcp"
    for k in ("3", "30"):
        r = subprocess.run([kiss, "suffix_sort", str(fa), "-k", k, "--output-lcp", str(lcp)], capture_output=True, text=True)
        assert r.returncode != 0
        assert "--output-lcp needs the exact suffix array" in r.stderr, r.stderr
        assert "suffix sorting elapsed" not in r.stderr and not lcp.exists()
    r = subprocess.run([kiss, "suffix_sort", str(fa), "-k", "-1", "--gpus", "2", "--output-lcp", str(lcp)],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "one device only" in r.stderr


# (file text, bases by the device parser's rule of fasta.hip): a line that begins with '>' is a header unless the line
# before it was one; a '>' inside a line is a base
FASTA_EDGE_CASES = [(">h\n>AAAAAAAAAA\nAAAA\n", 15), (">h\nAC>GTACGTAC\n", 11), (">a\n>b\n>c\nAC\n", 4),
                    (">a\n>b\n>c\n>d\nAC\n", 6), (">h\nACGT\n>h2\n>CC\nG", 8), ("AC>GT\n>ACGT\n", 10)]


@pytest.mark.parametrize("text,n", FASTA_EDGE_CASES)
def test_cli_bounded_k_check_counts_bases_as_the_parser_does(tmp_path, text, n):
    # k = n - 1 is refused on the host; k = n passes the check (and then needs a device: no LCP message either way)
    kiss = os.path.join(ROOT, "kiss_amd", "kiss")
    fa = tmp_path / "x.fa"
    fa.write_bytes(text.encode())
    lcp = tmp_path / "lcp"
    r = subprocess.run([kiss, "suffix_sort", str(fa), "-k", str(n - 1), "--output-lcp", str(lcp)], capture_output=True,
                       text=True)
    assert r.returncode != 0 and "--output-lcp needs the exact suffix array" in r.stderr, r.stderr
    r = subprocess.run([kiss, "suffix_sort", str(fa), "-k", str(n), "--output-lcp", str(lcp)], capture_output=True,
                       text=True)
    assert "--output-lcp needs the exact suffix array" not in r.stderr, r.stderr
