// cli_bam_index.hpp -- `kiss fmindex_query ... --sam --bam FILE --bam-sort --bam-index`: the host side of the BAI index that the
// command line writes beside a sorted file (kiss --help-bam).  Plain host C++ that needs no library: where the index
// goes, the one refusal that the option table cannot express, and what the framing has to leave behind for it -- the bytes of the
// file in front of the first record block and, with --bam-compress, the offset of every block.  tests/cli_bam_index_check.cpp
// compiles this file alone.  The index itself is the library's (include/kiss_hip_bai.h): cli_reads.hpp calls it once, behind the
// sort and before anything is written to FILE.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace kiss_cli {

// FILE.bai
inline std::string bam_index_path(const std::string &bam) { return bam + ".bai"; }

// --bam-index goes with --bam FILE --bam-sort: the option table says so (--bam-index goes with --bam-sort, which goes with --bam).
// What the table cannot say: an index of what goes to stdout has no name
inline void bam_index_options(bool bam_index, const std::string &bam)
{
    if (bam_index && bam == "-")
        throw std::runtime_error("--bam-index writes FILE.bai beside --bam FILE: it does not go with --bam - (kiss --help-bam)");
}

// how many blocks of `block_bytes` payload bytes hold n bytes
inline uint64_t bam_index_blocks(uint64_t n, uint64_t block_bytes)
{
    if (block_bytes == 0) throw std::logic_error("bam_index_blocks: no block size");
    return (n + block_bytes - 1) / block_bytes;
}

// what the framing of a sorted file leaves for the index
struct BamIndexFrame {
    uint64_t file_base = 0;            // the bytes in front of the first record block: the framed header
    bool compressed = false;           // block_index holds the offsets (stored blocks need none)
    std::vector<uint64_t> block_index; // blocks + 1 entries from 0, over the record blocks
    // room for the offsets of the blocks of n payload bytes; -> the entries the framing call may write
    uint64_t room(uint64_t n, uint64_t block_bytes)
    {
        compressed = true;
        block_index.assign(bam_index_blocks(n, block_bytes) + 1, 0);
        return block_index.size();
    }
    // the offsets as the framing call left them: from 0, never decreasing, `framed` bytes in all
    void check(uint64_t framed) const
    {
        if (!compressed) return;
        if (block_index.empty() || block_index.front() != 0 || block_index.back() != framed)
            throw std::logic_error("BamIndexFrame: the block index does not cover the framed bytes");
        for (size_t b = 1; b < block_index.size(); b++)
            if (block_index[b] < block_index[b - 1]) throw std::logic_error("BamIndexFrame: the block index decreases");
    }
    const uint64_t *offsets() const { return compressed ? block_index.data() : nullptr; }
};

} // namespace kiss_cli
