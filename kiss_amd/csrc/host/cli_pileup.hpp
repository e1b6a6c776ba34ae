// cli_pileup.hpp -- `kiss fmindex_query --seeds READS ... --sam --pileup FILE`: the lines of the pileup file, from the planes that
// kiss_hip_fmi_pileup_host summed on the device (include/kiss_hip_pileup.h: 8 planes of n u32, plane-major: COV, ALT_A, ALT_C,
// ALT_G, ALT_T, ALT_N, DEL, INS).  Standard headers alone, so that a test compiles it without the library
// (tests/test_cli_pileup.py).
// One line per text position j with COV + DEL + INS > 0, tab-separated:
//   RNAME  POS  REF  COV  A  C  G  T  N  DEL  INS
// RNAME: the record of the reference that holds j ('*' without records); POS: 1-based inside that record; REF: the text's letter
// ('N' for a byte above 3); COV: the aligned read bases over j; A C G T N: those bases by letter, the ones equal to the text
// included (they number COV minus the five ALT planes); DEL: the reads that delete j; INS: the insertions directly behind j.
// The depth in samtools' sense is COV + DEL.
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

namespace kiss_cli {

// the lines of the positions [from, to) of a text of n bases; bounds: the starts of the records plus n (names.size() + 1 values,
// the first 0), records without bases left out as the SAM header leaves them out
inline void pileup_lines(std::string &out, const uint32_t *planes, uint64_t n, const uint8_t *text, const std::vector<std::string> &names,
                         const std::vector<uint64_t> &bounds, uint64_t from, uint64_t to)
{
    const uint64_t R = names.size();
    uint64_t r = 0;
    for (uint64_t j = from; j < to && j < n; j++) {
        const uint32_t cov = planes[j], del = planes[6 * n + j], ins = planes[7 * n + j];
        if (!(cov | del | ins)) continue;
        while (r + 1 < R && bounds[r + 1] <= j) r++;
        uint32_t base[5], alts = 0;
        for (int b = 0; b < 5; b++) alts += base[b] = planes[(uint64_t)(1 + b) * n + j];
        const uint8_t t = text[j];
        if (t <= 3) base[t] += cov - alts;
        out += R ? names[r] : std::string("*");
        out += '\t' + std::to_string(j - (R ? bounds[r] : 0) + 1) + '\t' + "ACGTN"[t <= 3 ? t : 4] + '\t' + std::to_string(cov);
        for (int b = 0; b < 5; b++) out += '\t' + std::to_string(base[b]);
        out += '\t' + std::to_string(del) + '\t' + std::to_string(ins) + '\n';
    }
}

// the file, written a stretch of positions at a time
inline void write_pileup(std::FILE *f, const std::string &path, const uint32_t *planes, uint64_t n, const uint8_t *text,
                         const std::vector<std::string> &names, const std::vector<uint64_t> &bounds)
{
    std::string out;
    for (uint64_t from = 0; from < n; from += 1u << 16) {
        out.clear();
        pileup_lines(out, planes, n, text, names, bounds, from, from + (1u << 16));
        if (std::fwrite(out.data(), 1, out.size(), f) != out.size()) throw std::runtime_error("cannot write " + path);
    }
    if (std::fflush(f) != 0) throw std::runtime_error("cannot write " + path);
}

} // namespace kiss_cli
