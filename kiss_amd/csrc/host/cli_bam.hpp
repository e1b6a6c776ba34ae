// cli_bam.hpp -- `kiss fmindex_query ... --sam --bam FILE`: the BAM header in front of the records (kiss --help-bam; DESIGN.md
// 4.22).  Plain host C++ that needs no library: the magic, the text of the SAM header, and the records of the reference with their
// lengths, unframed -- what kiss_amd.bam_writer.bam_header gives (tests/test_bam_model.py compiles this file alone and holds the two
// against each other).  The framing of the header, and the records and blocks of every batch, are the library's
// (include/kiss_hip_bam.h): cli_reads.hpp calls it.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace kiss_cli {

inline void bam_put_i32(std::string &out, int64_t v)
{
    const uint32_t u = (uint32_t)v;
    for (int k = 0; k < 4; k++) out.push_back((char)(uint8_t)(u >> (8 * k)));
}

// text: the header lines of the SAM output; names and bounds (R + 1 starts): the records of the reference
inline std::string bam_header(const std::string &text, const std::vector<std::string> &names, const std::vector<uint64_t> &bounds)
{
    if (bounds.size() != names.size() + 1) throw std::logic_error("bam_header: bounds has one entry more than names");
    if (text.size() >= (1ull << 31) || names.size() >= (1ull << 31)) throw std::runtime_error("--bam: the header text or the records are more than a BAM header holds");
    std::string out("BAM\1", 4);
    bam_put_i32(out, (int64_t)text.size());
    out += text;
    bam_put_i32(out, (int64_t)names.size());
    for (size_t r = 0; r < names.size(); r++) {
        const uint64_t len = bounds[r + 1] - bounds[r];
        if (bounds[r + 1] < bounds[r] || len >= (1ull << 31) || names[r].size() + 1 >= (1ull << 31))
            throw std::runtime_error("--bam: record " + names[r] + " has " + std::to_string(len) + " bases: a BAM header holds fewer than 2^31");
        bam_put_i32(out, (int64_t)names[r].size() + 1);
        out += names[r];
        out.push_back('\0');
        bam_put_i32(out, (int64_t)len);
    }
    return out;
}

} // namespace kiss_cli
