// The BAM header of the command line (kiss_amd/csrc/host/cli_bam.hpp), compiled alone: tests/test_bam_model.py holds its bytes
// against kiss_amd.bam_writer.bam_header.  cli_bam_check TEXT_FILE R NAME... BOUND... writes the header to stdout; a header that
// cannot be written is one line on stderr and status 2.
#include "kiss_amd/csrc/host/cli_bam.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>

int main(int argc, char **argv)
{
    if (argc < 3) return 1;
    std::ifstream in(argv[1], std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const size_t R = std::strtoull(argv[2], nullptr, 10);
    if ((size_t)argc != 3 + R + R + 1) return 1;
    std::vector<std::string> names;
    std::vector<uint64_t> bounds;
    for (size_t r = 0; r < R; r++) names.push_back(argv[3 + r]);
    for (size_t r = 0; r <= R; r++) bounds.push_back(std::strtoull(argv[3 + R + r], nullptr, 10));
    try {
        const std::string h = kiss_cli::bam_header(text, names, bounds);
        std::fwrite(h.data(), 1, h.size(), stdout);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 0;
}
