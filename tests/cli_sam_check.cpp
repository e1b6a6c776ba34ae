// The SAM line functions of kiss_amd/csrc/host/cli_format.hpp on States read from a file (tests/test_fm_sam_model.py writes the
// file and holds tests/fm_sam_model.py against what this prints): cli_format.hpp alone, no libkiss_hip.
// File: u64 batches; per batch u64 paired, has_qual, has_md, has_source, first_alns, R, Q, C, H, then the arrays in the order read
// below (a string: u64 length, bytes).  Output per batch: its bytes in decimal, '\n', the lines.
#include "kiss_amd/csrc/host/cli_format.hpp"

#include <cstring>

using namespace kiss_cli;

static std::vector<uint8_t> file;
static size_t at = 0;

static void take(void *dst, size_t bytes)
{
    if (at + bytes > file.size()) throw std::runtime_error("the file ends inside a batch");
    if (bytes) std::memcpy(dst, file.data() + at, bytes);
    at += bytes;
}
static uint64_t u64()
{
    uint64_t v;
    take(&v, 8);
    return v;
}
template <class T> static void array(std::vector<T> &v, uint64_t count)
{
    v.resize(count);
    take(v.data(), count * sizeof(T));
}
static std::string text()
{
    std::string s(u64(), ' ');
    take(&s[0], s.size());
    return s;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    file.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint64_t batches = u64();
    for (uint64_t k = 0; k < batches; k++) {
        State s;
        const uint64_t paired = u64(), has_qual = u64(), has_md = u64(), has_source = u64();
        s.first_alns = u64();
        const uint64_t R = u64(), Q = u64(), C = u64(), H = u64();
        s.Q = Q;
        array(s.rd.ridx, Q + 1);
        array(s.rd.reads, s.rd.ridx[Q]);
        s.rd.has_qual = has_qual != 0;
        if (has_qual) array(s.rd.qual, s.rd.ridx[Q]);
        for (uint64_t q = 0; q < Q; q++) s.rd.names.push_back(text());
        array(s.al.alns, C);
        array(s.al.oidx, C + 1);
        array(s.al.cigar, s.al.oidx[C]);
        array(s.hits, H);
        array(s.hidx, Q + 1);
        if (paired) array(s.pairs, Q / 2);
        if (has_source) array(s.source, C);
        if (has_md) {
            array(s.midx, H + 1);
            array(s.md, s.midx[H]);
        }
        for (uint64_t r = 0; r < R; r++) s.ref.names.push_back(text());
        array(s.ref.bounds, R + 1);
        std::string out;
        for (uint64_t i = 0; i < (paired ? Q / 2 : Q); i++) {
            if (paired) sam_pair_lines(out, s, i, s.pairs[i]);
            else sam_read_lines(out, s, i);
        }
        std::printf("%llu\n", (unsigned long long)out.size());
        std::fwrite(out.data(), 1, out.size(), stdout);
    }
    return at == file.size() ? 0 : 3;
}
