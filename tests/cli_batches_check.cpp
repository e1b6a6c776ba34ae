// The chunk reader of `kiss fmindex_query --batch-reads` (kiss_amd/csrc/host/cli_batches.hpp) without the library
// (tests/test_cli_batches.py): `cli_batches_check FILE FORMAT CHUNK_BYTES BATCH_READS` feeds FILE through a ChunkReader whose part
// call is host_part() below, the definition of include/kiss_hip_reads_part.h as plain loops on the host, and prints per batch
// `batch FIRST RECORDS FORMAT`, then per read `name codes qual` (qual: - without qualities).  An error ends it with status 3 and
// the message on stderr, behind the batches before it.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "kiss_amd/csrc/host/cli_batches.hpp"

namespace {

struct Line { uint64_t beg, end, next; }; // [beg, end) after the '\r' strip; next: behind its '\n' (or the chunk's end)

uint8_t code_of(uint8_t c)
{
    switch (c) {
    case 'A': case 'a': return 0;
    case 'C': case 'c': return 1;
    case 'G': case 'g': return 2;
    case 'T': case 't': return 3;
    default: return 4;
    }
}

int host_part(const uint8_t *raw, uint64_t bytes, int format, int final, uint64_t max_records, uint8_t *codes, uint8_t *qual, uint64_t bases_capacity,
              uint64_t *read_index, uint64_t *name_off, uint32_t *name_len, uint64_t reads_capacity, kiss_hip_reads_part_report *rep)
{
    *rep = kiss_hip_reads_part_report{};
    kiss_hip_reads_report &p = rep->parsed;
    if (format == KISS_HIP_READS_AUTO) format = bytes && raw[0] == '@' ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_LINES;
    p.format = (uint32_t)format;
    p.has_qual = format == KISS_HIP_READS_FASTQ;
    std::vector<Line> lines; // the complete lines
    for (uint64_t beg = 0; beg < bytes;) {
        uint64_t end = beg;
        while (end < bytes && raw[end] != '\n') end++;
        if (end == bytes && !final) break; // the piece behind the last '\n'
        lines.push_back({beg, end > beg && raw[end - 1] == '\r' ? end - 1 : end, std::min(end + 1, bytes)});
        beg = end + 1;
    }
    const auto is_read = [&](const Line &l) { return l.end > l.beg && raw[l.beg] != '>'; };
    uint64_t kept = lines.size(), complete = 0;
    if (format == KISS_HIP_READS_FASTQ) {
        while (kept && lines[kept - 1].beg == lines[kept - 1].end) kept--;
        complete = final ? (kept + 3) / 4 : kept / 4;
    } else {
        for (const Line &l : lines) complete += is_read(l);
    }
    const uint64_t records = max_records ? std::min(max_records, complete) : complete;
    const bool whole = final && records == complete;
    uint64_t used = whole ? bytes : 0, taken = whole ? (format == KISS_HIP_READS_FASTQ ? kept : lines.size()) : 0; // lines of the prefix
    if (!whole && records && format == KISS_HIP_READS_FASTQ) taken = 4 * records, used = lines[taken - 1].next;
    if (!whole && records && format == KISS_HIP_READS_LINES)
        for (uint64_t k = 0, seen = 0; seen < records; k++)
            if (is_read(lines[k]) && ++seen == records) taken = k + 1, used = lines[k].next;
    rep->records_complete = complete, rep->records = records, rep->bytes_used = used;
    p.lines = taken;
    // the prefix: the sequence, quality and name spans of its reads
    struct Read { Line seq, qual; uint64_t noff; uint32_t nlen; };
    std::vector<Read> reads;
    const auto name_of = [&](const Line &l, Read &r) {
        uint64_t j = l.beg + 1;
        while (j < l.end && raw[j] != ' ' && raw[j] != '\t') j++;
        r.noff = l.beg + 1, r.nlen = (uint32_t)(j - (l.beg + 1));
    };
    if (format == KISS_HIP_READS_FASTQ) {
        for (uint64_t r = 0; r < (taken + 3) / 4; r++) {
            const Line *rec = &lines[4 * r];
            uint32_t kind = 0;
            if (4 * r + 4 > taken) kind = 4;
            else if (rec[0].beg == rec[0].end || raw[rec[0].beg] != '@') kind = 1;
            else if (rec[2].beg == rec[2].end || raw[rec[2].beg] != '+') kind = 2;
            else if (rec[1].end - rec[1].beg != rec[3].end - rec[3].beg) kind = 3;
            if (kind) {
                if (!p.bad_records++) p.first_bad = r, p.first_bad_kind = kind;
                continue;
            }
            if (rec[1].beg == rec[1].end && !p.empty_reads++) p.first_empty = r;
            Read rd{rec[1], rec[3], 0, 0};
            name_of(rec[0], rd);
            reads.push_back(rd);
        }
    } else {
        for (uint64_t k = 0; k < taken; k++) {
            if (!is_read(lines[k])) continue;
            Read rd{lines[k], lines[k], 0, 0};
            if (k && lines[k - 1].end > lines[k - 1].beg && raw[lines[k - 1].beg] == '>') name_of(lines[k - 1], rd);
            reads.push_back(rd);
        }
    }
    if (p.bad_records) return KISS_HIP_E_INVALID;
    p.reads = reads.size();
    for (const Read &r : reads) p.bases += r.seq.end - r.seq.beg;
    if (p.reads > reads_capacity || p.bases > bases_capacity) return KISS_HIP_E_INVALID;
    uint64_t at = 0;
    read_index[0] = 0;
    for (uint64_t q = 0; q < reads.size(); q++) {
        const Read &r = reads[q];
        for (uint64_t j = r.seq.beg; j < r.seq.end; j++, at++) {
            codes[at] = code_of(raw[j]);
            p.no_base += codes[at] == 4;
            if (p.has_qual && qual) qual[at] = raw[r.qual.beg + (j - r.seq.beg)];
        }
        read_index[q + 1] = at;
        if (name_off) name_off[q] = r.noff, name_len[q] = r.nlen;
    }
    return KISS_HIP_OK;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const int format = !std::strcmp(argv[2], "lines") ? KISS_HIP_READS_LINES : !std::strcmp(argv[2], "fastq") ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_AUTO;
    const uint64_t chunk = std::strtoull(argv[3], nullptr, 10), batch_reads = std::strtoull(argv[4], nullptr, 10);
    try {
        kiss_cli::ChunkReader<decltype(&host_part)> reader(argv[1], format, chunk, true, &host_part);
        while (const uint64_t K = reader.ready(batch_reads)) {
            const uint64_t first = reader.first();
            const kiss_cli::ReadFile f = reader.take(K);
            if (f.ridx.size() != K + 1 || f.names.size() != K || reader.first() != first + K) return 1;
            std::cout << "batch " << first << ' ' << K << ' ' << (reader.format() == KISS_HIP_READS_FASTQ ? "fastq" : "lines") << '\n';
            for (uint64_t q = 0; q < K; q++) {
                std::cout << f.names[q] << ' ';
                for (uint64_t i = f.ridx[q]; i < f.ridx[q + 1]; i++) std::cout << (int)f.reads[i];
                std::cout << ' ';
                if (!f.has_qual) std::cout << '-';
                for (uint64_t i = f.ridx[q]; f.has_qual && i < f.ridx[q + 1]; i++) std::cout << std::hex << (int)f.qual[i] << std::dec << '.';
                std::cout << '\n';
            }
            std::cout.flush();
        }
        return 0;
    } catch (const std::exception &e) {
        std::cerr << e.what() << '\n';
        return 3;
    }
}
