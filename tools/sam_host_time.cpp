// The host writer of `kiss fmindex_query --sam` timed on a batch that tools/bench_sam.py dumped (--dump DIR), so that the two
// writers are measured on the same arrays: cli_format.hpp alone, as tests/cli_sam_check.cpp, and the file format that program
// reads (one batch).  sam_lines' work -- sam_read_lines / sam_pair_lines of every read or pair -- into one string, on one
// thread, best of five, one JSON line on stdout.
// build: g++ -O3 -std=c++17 -I. tools/sam_host_time.cpp -o sam_host_time        usage: sam_host_time FILE.state
#include "kiss_amd/csrc/host/cli_format.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>

using namespace kiss_cli;

static std::vector<uint8_t> file;
static size_t at = 0;

static void take(void *dst, size_t bytes)
{
    if (at + bytes > file.size()) throw std::runtime_error("the file ends inside the batch");
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
    if (u64() != 1) return 3; // (one batch)
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
    if (at != file.size()) return 3;
    double best = 1e30, all[5];
    size_t bytes = 0, lines = 0;
    for (int k = 0; k < 5; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        std::string out;
        for (uint64_t i = 0; i < (paired ? Q / 2 : Q); i++) {
            if (paired) sam_pair_lines(out, s, i, s.pairs[i]);
            else sam_read_lines(out, s, i);
        }
        all[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        best = all[k] < best ? all[k] : best;
        bytes = out.size();
        lines = (size_t)std::count(out.begin(), out.end(), '\n');
    }
    std::printf("{\"host_ms_best\": %.3f, \"host_ms_all\": [%.3f, %.3f, %.3f, %.3f, %.3f], \"lines\": %zu, \"sam_bytes\": %zu, \"threads\": 1}\n", best,
                all[0], all[1], all[2], all[3], all[4], lines, bytes);
    return 0;
}
