// The pileup writer of kiss_amd/csrc/host/cli_pileup.hpp on planes read from a file (tests/test_cli_pileup.py writes the file
// and holds lines made from the planes of tests/fm_pileup_model.py against what this prints): the header alone, no libkiss_hip.
// File: u64 n, u64 R, R names (u64 length, bytes), R + 1 u64 bounds, n text bytes, 8 n u32 planes.  Output: the lines.
#include "kiss_amd/csrc/host/cli_pileup.hpp"

#include <cstring>
#include <fstream>
#include <iterator>

using namespace kiss_cli;

static std::vector<uint8_t> file;
static size_t at = 0;

static void take(void *dst, size_t bytes)
{
    if (at + bytes > file.size()) throw std::runtime_error("the file ends inside an array");
    if (bytes) std::memcpy(dst, file.data() + at, bytes);
    at += bytes;
}
static uint64_t u64()
{
    uint64_t v;
    take(&v, 8);
    return v;
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    file.assign((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const uint64_t n = u64(), R = u64();
    std::vector<std::string> names;
    for (uint64_t r = 0; r < R; r++) {
        std::string s(u64(), ' ');
        take(&s[0], s.size());
        names.push_back(s);
    }
    std::vector<uint64_t> bounds(R + 1);
    take(bounds.data(), 8 * (R + 1));
    std::vector<uint8_t> text(n);
    take(text.data(), n);
    std::vector<uint32_t> planes(8 * n);
    take(planes.data(), 32 * n);
    write_pileup(stdout, "stdout", planes.data(), n, text.data(), names, bounds);
    return at == file.size() ? 0 : 3;
}
