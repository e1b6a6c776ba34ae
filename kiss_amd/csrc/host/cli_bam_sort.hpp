// cli_bam_sort.hpp -- `kiss fmindex_query ... --sam --bam FILE --bam-sort`: what the command line keeps of the batches until the
// whole file can be sorted (kiss --help-bam).  Plain host C++ that needs no library: the unframed records of every
// batch one after the other, the CSR over all of them (the index of a batch rebased onto the bytes in front of it), and the word of
// the @HD line that says which order the file has.  tests/cli_bam_sort_check.cpp compiles this file alone.  The sort itself is the
// library's (include/kiss_hip_bam_sort.h): cli_reads.hpp calls it once, behind the last batch.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace kiss_cli {

// the records of a file, batch after batch: bytes, and index with records() + 1 entries from 0
struct BamSortRecords {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> index{0};
    uint64_t records() const { return index.size() - 1; }
    // bam[0, n): the records of one batch; rec_index: its CSR, `count` + 1 entries from 0 (null with count 0)
    void add(const uint8_t *bam, uint64_t n, const uint64_t *rec_index, uint64_t count)
    {
        if (count == 0) {
            if (n) throw std::logic_error("BamSortRecords: bytes without records");
            return;
        }
        if (!bam || !rec_index || rec_index[0] != 0 || rec_index[count] != n) throw std::logic_error("BamSortRecords: the index does not cover the bytes");
        const uint64_t base = bytes.size();
        bytes.insert(bytes.end(), bam, bam + n);
        index.reserve(index.size() + count);
        for (uint64_t r = 1; r <= count; r++) {
            if (rec_index[r] < rec_index[r - 1]) throw std::logic_error("BamSortRecords: the index decreases");
            index.push_back(base + rec_index[r]);
        }
    }
};

// the header lines of the SAM output with SO:coordinate in the @HD line (nothing else changes)
inline std::string sam_header_coordinate(const std::string &text)
{
    static const std::string from = "SO:unsorted", to = "SO:coordinate";
    const size_t line_end = text.find('\n');
    const size_t at = text.find(from);
    if (text.compare(0, 3, "@HD") != 0 || at == std::string::npos || (line_end != std::string::npos && at > line_end))
        throw std::logic_error("sam_header_coordinate: no @HD line with SO:unsorted");
    return text.substr(0, at) + to + text.substr(at + from.size());
}

} // namespace kiss_cli
