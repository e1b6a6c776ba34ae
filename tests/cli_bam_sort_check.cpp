// What the command line keeps for --bam-sort (kiss_amd/csrc/host/cli_bam_sort.hpp), compiled alone with cli_bam.hpp:
// tests/test_cli_bam_sort_check.py feeds it batches and holds the answers against the straightforward concatenation and against
// kiss_amd.bam_writer.bam_header(sort_order="coordinate").
//   cli_bam_sort_check records FILE SIZES...  FILE holds the record bytes of all batches; SIZES is one word per batch, the bytes of
//     its records joined by commas ("-" for a batch without records).  The batches are added one by one, each with an index of its
//     own from 0; stdout: the count of records, the index entries, then the kept bytes as hex, one line each.
//   cli_bam_sort_check header TEXT_FILE R NAME... BOUND...  the BAM header over the text with SO:coordinate, on stdout; a text
//     without the @HD line is one line on stderr and status 2.
#include "kiss_amd/csrc/host/cli_bam.hpp"
#include "kiss_amd/csrc/host/cli_bam_sort.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>

static std::string slurp(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static int records(int argc, char **argv)
{
    const std::string all = slurp(argv[2]);
    kiss_cli::BamSortRecords kept;
    size_t at = 0;
    for (int k = 3; k < argc; k++) {
        std::vector<uint64_t> index{0};
        if (std::strcmp(argv[k], "-") != 0)
            for (const char *p = argv[k]; *p;) {
                char *end = nullptr;
                index.push_back(index.back() + std::strtoull(p, &end, 10));
                p = *end == ',' ? end + 1 : end;
            }
        const uint64_t n = index.back(), count = index.size() - 1;
        if (at + n > all.size()) return 1;
        // a batch of its own, at an address of its own: nothing of it may be kept by reference
        std::vector<uint8_t> batch(all.begin() + (long)at, all.begin() + (long)(at + n));
        kept.add(count ? batch.data() : nullptr, n, count ? index.data() : nullptr, count);
        at += n;
    }
    std::printf("%llu\n", (unsigned long long)kept.records());
    for (uint64_t x : kept.index) std::printf("%llu ", (unsigned long long)x);
    std::printf("\n");
    for (uint8_t b : kept.bytes) std::printf("%02x", b);
    std::printf("\n");
    return 0;
}

static int header(int argc, char **argv)
{
    const std::string text = slurp(argv[2]);
    const size_t R = std::strtoull(argv[3], nullptr, 10);
    if ((size_t)argc != 4 + R + R + 1) return 1;
    std::vector<std::string> names;
    std::vector<uint64_t> bounds;
    for (size_t r = 0; r < R; r++) names.push_back(argv[4 + r]);
    for (size_t r = 0; r <= R; r++) bounds.push_back(std::strtoull(argv[4 + R + r], nullptr, 10));
    const std::string h = kiss_cli::bam_header(kiss_cli::sam_header_coordinate(text), names, bounds);
    std::fwrite(h.data(), 1, h.size(), stdout);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc >= 3 && !std::strcmp(argv[1], "records")) return records(argc, argv);
        if (argc >= 4 && !std::strcmp(argv[1], "header")) return header(argc, argv);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 1;
}
