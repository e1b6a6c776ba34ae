// The two file parsers of `kiss fmindex_query --seeds ...` (tests/test_cli_format.py): `records FILE` prints the records of a
// reference file, one `name start end` per line; `reads FILE` and `reads_unnamed FILE` print the reads, one `name codes` per line.
#include <cstring>
#include <iostream>

#include "kiss_amd/csrc/host/cli_format.hpp"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    try {
    if (!std::strcmp(argv[1], "records")) {
        const kiss_cli::RefRecords r = kiss_cli::scan_records(argv[2]);
        for (size_t i = 0; i < r.names.size(); i++) std::cout << r.names[i] << ' ' << r.bounds[i] << ' ' << r.bounds[i + 1] << '\n';
        return r.bounds.size() == r.names.size() + 1 ? 0 : 1;
    }
    const bool names = !std::strcmp(argv[1], "reads");
    const kiss_cli::ReadFile f = kiss_cli::read_file(argv[2], names);
    if (f.names.size() != (names ? f.ridx.size() - 1 : 0)) return 1;
    for (size_t q = 0; q + 1 < f.ridx.size(); q++) {
        std::cout << (names ? f.names[q] : "-") << ' ';
        for (uint64_t i = f.ridx[q]; i < f.ridx[q + 1]; i++) std::cout << (int)f.reads[i];
        std::cout << '\n';
    }
    return 0;
    } catch (const std::exception &e) {
        std::cerr << e.what() << '\n';
        return 3;
    }
}
