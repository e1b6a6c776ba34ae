// The host side of --bam-index (kiss_amd/csrc/host/cli_bam_index.hpp), compiled alone: tests/test_cli_bam_index_check.py asks it
// where the index goes, which word of --bam it refuses and what the framing leaves for it.
//   cli_bam_index_check path FILE                      FILE.bai on stdout
//   cli_bam_index_check options INDEX BAM              (0 / 1, the word of --bam) "ok" on stdout, or the refusal as one line on
//     stderr and status 2
//   cli_bam_index_check blocks N BLOCK_BYTES           how many blocks hold N bytes
//   cli_bam_index_check frame N BLOCK_BYTES FRAMED OFFSET...  room(N, BLOCK_BYTES), then the offsets written into the room as a
//     framing call would (more than there is room for: status 1), then check(FRAMED); stdout: the entries of the room, then the
//     offsets as offsets() hands them on; a frame that was never given room says "stored"
#include "kiss_amd/csrc/host/cli_bam_index.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static unsigned long long num(const char *s) { return std::strtoull(s, nullptr, 10); }

static int frame(int argc, char **argv)
{
    kiss_cli::BamIndexFrame f;
    if (f.offsets() != nullptr) return 1;
    f.check(12345); // (stored blocks: nothing to hold against the bytes)
    if (argc == 2) {
        std::printf("stored\n");
        return 0;
    }
    const uint64_t entries = f.room(num(argv[2]), num(argv[3]));
    if ((uint64_t)(argc - 5) > entries) return 1;
    for (int k = 5; k < argc; k++) f.block_index[(size_t)(k - 5)] = num(argv[k]);
    f.check(num(argv[4]));
    std::printf("%llu\n", (unsigned long long)entries);
    for (uint64_t b = 0; b < entries; b++) std::printf("%llu ", (unsigned long long)f.offsets()[b]);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 3 && !std::strcmp(argv[1], "path")) {
            std::printf("%s", kiss_cli::bam_index_path(argv[2]).c_str());
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "options")) {
            kiss_cli::bam_index_options(num(argv[2]) != 0, argv[3]);
            std::printf("ok");
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "blocks")) {
            std::printf("%llu", (unsigned long long)kiss_cli::bam_index_blocks(num(argv[2]), num(argv[3])));
            return 0;
        }
        if ((argc == 2 || argc >= 5) && !std::strcmp(argv[1], "frame")) return frame(argc, argv);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    }
    return 1;
}
