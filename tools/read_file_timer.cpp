// The command line's host loader of read files, kiss_cli::read_file (kiss_amd/csrc/host/cli_format.hpp), timed on a file of one read
// per line: tools/bench_reads.py compiles this and holds the device parser against it.
// usage: read_file_timer FILE STEPS -> one line: reads bases ms ms ms ... (a warm-up call first, not printed)
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "../kiss_amd/csrc/host/cli_format.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int steps = std::atoi(argv[2]);
    kiss_cli::ReadFile f = kiss_cli::read_file(argv[1], true);
    std::printf("%llu %llu", (unsigned long long)(f.ridx.size() - 1), (unsigned long long)f.reads.size());
    for (int s = 0; s < steps; s++) {
        const auto t0 = std::chrono::steady_clock::now();
        f = kiss_cli::read_file(argv[1], true);
        std::printf(" %.3f", 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    std::printf("\n");
    return f.names.size() == f.ridx.size() - 1 ? 0 : 1;
}
