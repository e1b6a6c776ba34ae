"""The count pass of the induction counts class bytes four at a time (kiss_amd/csrc/induce_count.hpp: byte-wise 0/1 masks per
class, added into byte fields, summed once).  The header is plain C++ for host and device alike, so the arithmetic is held
against its byte-by-byte definition without a device: tests/induce_count_check.cpp, built here with AddressSanitizer and
UBSan and run as a program of its own -- every byte value 0 .. 15 in every byte position under all 16 emit masks, and
accumulations over a lane's nine words (and the most words the header allows) in which every field stands at its maximum."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packed_class_counts_equal_the_byte_by_byte_definition(tmp_path):
    exe = str(tmp_path / "induce_count_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", ROOT, os.path.join(ROOT, "tests", "induce_count_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr)
    word, cases = r.stdout.split()
    assert word == "ok" and int(cases) > 16 * 65536, r.stdout
