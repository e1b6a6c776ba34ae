// The host helpers of the FASTQ path of `kiss fmindex_query --seeds ...` (tests/test_reads_model.py), on a State made by hand: the
// names of reads from their spans in a file's bytes (the read number where a span is empty), /1 and /2 taken off the names of
// mates, and the QUAL column of the SAM lines -- forward, reversed on a FLAG 16 line, as read on a FLAG 4 line, * without
// qualities.  Calls no kiss_hip_* function.
#include <iostream>

#include "kiss_amd/csrc/host/cli_format.hpp"

using namespace kiss_cli;

int main()
{
    // names: spans into the bytes of a file
    const std::string text = "@first words\nACGT\n+\nIIII\n@\nAC\n+\n#!\n@pair/1\tx\nGG\n+\n;;\n";
    const std::vector<uint8_t> raw(text.begin(), text.end());
    const std::vector<uint64_t> off{1, 26, 36};
    const std::vector<uint32_t> len{5, 0, 6};
    for (const std::string &n : names_from_spans(raw, off, len, 3)) std::cout << "name " << n << '\n';
    for (std::string n : {"pair/1", "pair/2", "pair/3", "/1", "x/", "1", "", "a/1/2", "r0"}) {
        strip_mate_suffix(n);
        std::cout << "strip [" << n << "]\n";
    }

    // QUAL: two reads, one hit forward, one reverse, one read unmapped; then the same without qualities
    State s;
    const std::string letters[3] = {"ACGTA", "AACCG", "TTN"}, quals[3] = {"ABCDE", "!#$%&", "@+>"};
    for (int q = 0; q < 3; q++) {
        for (char c : letters[q]) s.rd.reads.push_back(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4);
        for (char c : quals[q]) s.rd.qual.push_back((uint8_t)c);
        s.rd.ridx.push_back(s.rd.reads.size());
        s.rd.names.push_back("r" + std::to_string(q));
    }
    s.Q = s.V = 3;
    s.ref.names = {"chr"};
    s.ref.bounds = {0, 100};
    kiss_hip_aln a{};
    a.score = 5, a.rbeg = 0, a.rend = 5, a.tbeg = 10, a.tend = 15, a.matches = 5;
    s.al.alns = {a, a};
    s.al.cigar = {5u << 4, 5u << 4};
    s.al.oidx = {0, 1, 2};
    kiss_hip_hit h0{}, h1{};
    h0.aln = 0, h0.mapq = 60, h0.score = 5;
    h1.aln = 1, h1.mapq = 30, h1.score = 5, h1.flags = KISS_HIP_HIT_REVERSE;
    s.hits = {h0, h1};
    s.hidx = {0, 1, 2, 2};
    for (int pass = 0; pass < 2; pass++) {
        s.rd.has_qual = pass == 0;
        std::string out;
        for (uint64_t q = 0; q < 3; q++) sam_read_lines(out, s, q);
        std::cout << out;
        std::cout << "qual " << read_qual(s.rd, 0, false) << ' ' << read_qual(s.rd, 0, true) << '\n';
    }
    return 0;
}
