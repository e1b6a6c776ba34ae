// cli_reads.hpp -- `kiss fmindex_query --seeds READS ...`: the read-mapping pipeline.  One State (cli_format.hpp), filled stage by
// stage; a stage is a function of (Args, State) around its library call; map_reads() at the end runs them and leaves after the
// last one the command line asks for, with the printer of cli_format.hpp for what that made.  The read files are parsed on the
// device (kiss_hip_reads.h): one read per line, or FASTQ, whose qualities reach the QUAL column of the SAM.
#pragma once
#include "cli_common.hpp"
#include "cli_format.hpp"
#include "cli_batches.hpp"
#include "cli_pileup.hpp"
#include "cli_bam.hpp"
#include "cli_bam_sort.hpp"
#include "cli_bam_index.hpp"
#include "../../../include/kiss_hip_reads.h"
#include "../../../include/kiss_hip_md.h"
#include "../../../include/kiss_hip_insert.h"
#include "../../../include/kiss_hip_sam.h"
#include "../../../include/kiss_hip_bam.h"
#include "../../../include/kiss_hip_bam_sort.h"
#include "../../../include/kiss_hip_markdup.h"
#include "../../../include/kiss_hip_bai.h"
#include "../../../include/kiss_hip_deflate.h"
#include <iterator>

namespace kiss_cli {

// The size-then-fill protocol of the chain, align and rescue calls: call(capacity) is made with capacity 0; if it answers
// KISS_HIP_E_INVALID and its report now says how many entries it needs, `out` grows to that and the call is made once more.
template <class T, class Call> int sized_call(std::vector<T> &out, const uint64_t &needed, Call call)
{
    int rc = call(uint64_t(0));
    if (rc == KISS_HIP_E_INVALID && needed) {
        out.resize(needed);
        rc = call(needed);
    }
    return rc;
}

// One file of reads parsed on the device (kiss_hip_reads_parse_host, size then fill): the codes, the index, the qualities of a FASTQ
// file, and with_names the names from their spans in the file; *format: the one that was parsed.  The host reads the file
// into memory and looks at no byte of it but the names'.
inline ReadFile parse_read_file(const Args &a, const std::string &path, bool with_names, int *format)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    std::vector<uint8_t> raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    raw.reserve(1); // (a pointer that is not NULL)
    const int wanted = a.reads_format == "lines" ? KISS_HIP_READS_LINES : a.reads_format == "fastq" ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_AUTO;
    ReadFile f;
    kiss_hip_reads_report rep{};
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    const auto call = [&](uint64_t bases, uint64_t reads) {
        f.reads.resize(bases + 1);
        f.qual.resize(bases + 1);
        f.ridx.assign(reads + 1, 0);
        off.assign(reads + 1, 0);
        len.assign(reads + 1, 0);
        return kiss_hip_reads_parse_host(raw.data(), raw.size(), wanted, f.reads.data(), f.qual.data(), bases, f.ridx.data(),
                                         with_names ? off.data() : nullptr, with_names ? len.data() : nullptr, reads, &rep, a.device);
    };
    int rc = call(0, 0);
    if (rc == KISS_HIP_E_INVALID && !rep.bad_records && (rep.reads || rep.bases)) rc = call(rep.bases, rep.reads);
    if (rc == KISS_HIP_E_INVALID && rep.bad_records) {
        throw std::runtime_error("fmindex_query --seeds: " + path + " is no FASTQ file: " + std::to_string(rep.bad_records) +
                                 " bad records, the first is record " + std::to_string(rep.first_bad) + ": " + fastq_bad_kind(rep.first_bad_kind));
    }
    check(rc, "kiss_hip_reads_parse_host");
    if (rep.empty_reads)
        throw std::runtime_error("fmindex_query --seeds: read " + std::to_string(rep.first_empty) + " of " + path + " has no bases (" +
                                 std::to_string(rep.empty_reads) + " such reads)");
    f.has_qual = rep.has_qual != 0;
    f.reads.resize(rep.bases);
    f.qual.resize(f.has_qual ? rep.bases : 0);
    if (with_names) f.names = names_from_spans(raw, off, len, rep.reads);
    *format = (int)rep.format;
    return f;
}

// Read p of `first` and read p of `second`, P of each, as reads 2 p and 2 p + 1 of one batch (kiss_hip_reads_interleave_host); with
// names, those of FASTQ mates without /1 and /2
inline ReadFile interleave_mates(const Args &a, ReadFile &first, ReadFile &second, int format)
{
    const uint64_t P = first.ridx.size() - 1;
    ReadFile rd;
    rd.has_qual = first.has_qual;
    uint64_t bases = first.reads.size() + second.reads.size();
    rd.reads.resize(bases + 1);
    rd.qual.resize(bases + 1);
    rd.ridx.assign(2 * P + 1, 0);
    first.reads.reserve(1), second.reads.reserve(1), first.qual.reserve(1), second.qual.reserve(1);
    check(kiss_hip_reads_interleave_host(first.reads.data(), first.ridx.data(), first.has_qual ? first.qual.data() : nullptr, P, second.reads.data(),
                                         second.ridx.data(), first.has_qual ? second.qual.data() : nullptr, P, rd.reads.data(),
                                         rd.ridx.data(), first.has_qual ? rd.qual.data() : nullptr, bases, &bases, a.device),
          "kiss_hip_reads_interleave_host");
    rd.reads.resize(bases);
    rd.qual.resize(first.has_qual ? bases : 0);
    for (uint64_t p = 0; p < P && a.sam; p++)
        for (ReadFile *f : {&first, &second}) {
            if (format == KISS_HIP_READS_FASTQ) strip_mate_suffix(f->names[p]);
            rd.names.push_back(f->names[p]);
        }
    return rd;
}

[[noreturn]] inline void refuse_formats(const Args &a)
{
    throw std::runtime_error("fmindex_query --mates: " + a.seeds + " and " + a.mates + " differ in format (one is FASTQ, one has a read per line): "
                             "name it with --reads-format");
}

// READS, with --mates READS2 interleaved with it
inline void load_reads(const Args &a, State &s)
{
    int format = 0;
    s.rd = parse_read_file(a, a.seeds, a.sam, &format);
    if (!a.mates.empty()) { // reads 2 p and 2 p + 1 of the batch are read p of either file
        int format2 = 0;
        ReadFile first = std::move(s.rd), second = parse_read_file(a, a.mates, a.sam, &format2);
        const uint64_t P = first.ridx.size() - 1;
        if (second.ridx.size() - 1 != P)
            throw std::runtime_error("fmindex_query --mates: " + a.seeds + " has " + std::to_string(P) + " reads, " + a.mates + " has " +
                                     std::to_string(second.ridx.size() - 1) + " reads: a pair has one of each");
        if (format != format2) refuse_formats(a);
        s.rd = interleave_mates(a, first, second, format);
    }
    s.Q = s.rd.ridx.size() - 1;
    s.V = a.both_strands ? 2 * s.Q : s.Q;
}

// (its own protocol: the first call passes no position arrays, returns OK and sizes them)
inline void find_seeds(const Args &a, State &s)
{
    const uint64_t bases = (a.both_strands ? 2 : 1) * (uint64_t)s.rd.reads.size();
    s.seeds.resize(bases + 1);
    s.sidx.assign(s.V + 1, 0);
    const auto call = [&](uint32_t *pos, uint64_t *pidx, uint64_t capacity) {
        return kiss_hip_fmi_seeds_host(&s.index, s.rd.reads.data(), s.rd.ridx.data(), s.Q, a.min_seed_len, a.max_seed_len, a.max_occ, a.both_strands,
                                       nullptr, s.seeds.data(), s.sidx.data(), bases, pos, pidx, capacity, &s.seed_rep, a.device);
    };
    check(call(nullptr, nullptr, 0), "kiss_hip_fmi_seeds_host");
    s.pos.resize(s.seed_rep.positions + 1);
    s.pidx.resize(s.seed_rep.seeds + 1);
    const int rc = call(s.pos.data(), s.pidx.data(), s.seed_rep.positions);
    if (rc == KISS_HIP_E_INVALID && s.seed_rep.walk_failures)
        throw std::runtime_error("fmindex_query --seeds: " + std::to_string(s.seed_rep.walk_failures) +
                                 " rows of the index reached no sampled row: the positions need an index built with "
                                 "fmindex_build --exact");
    check(rc, "kiss_hip_fmi_seeds_host");
}

// --chain: the positions of the seeds of a virtual read chained into candidate loci
inline void chain_seeds(const Args &a, State &s)
{
    s.ch.chains.resize(1);
    s.ch.cidx.assign(s.V + 1, 0);
    check(sized_call(s.ch.chains, s.chain_rep.chains, [&](uint64_t capacity) {
              return kiss_hip_fmi_chain_host(s.seeds.data(), s.sidx.data(), s.V, s.pos.data(), s.pidx.data(), &a.chain_params, s.ch.chains.data(),
                                             s.ch.cidx.data(), capacity, nullptr, nullptr, 0, &s.chain_rep, a.device);
          }),
          "kiss_hip_fmi_chain_host");
}

// the C chains `ch` of the reads aligned to the text into `al`; option: the one named when the call refuses the batch
inline void align(const Args &a, const State &s, int both_strands, const Chains &ch, uint64_t C, Alignments &al, const char *option)
{
    al.alns.resize(C + 1);
    al.cigar.resize(1);
    al.oidx.assign(C + 1, 0);
    const int rc = sized_call(al.cigar, al.rep.cigar_ops, [&](uint64_t capacity) {
        return kiss_hip_fmi_align_host(s.S.data(), s.S.size(), s.rd.reads.data(), s.rd.ridx.data(), s.Q, both_strands, ch.chains.data(), ch.cidx.data(),
                                       &a.align_params, al.alns.data(), C, al.cigar.data(), al.oidx.data(), capacity, &al.rep, a.device);
    });
    if (rc == KISS_HIP_E_UNSUPPORTED && al.rep.cells)
        throw std::runtime_error(std::string("fmindex_query ") + option + ": " + std::to_string(al.rep.cells) +
                                 " DP cells are more than one call holds: split the reads");
    check(rc, "kiss_hip_fmi_align_host");
}

// --align: the text loaded as the index was built from it, every chain aligned to it
inline void load_text(const Args &a, State &s)
{
    s.S = DeviceText(a.fasta, a.device).to_host();
    s.S.reserve(1); // (a pointer that is not NULL)
}
inline void align_chains(const Args &a, State &s)
{
    load_text(a, s);
    align(a, s, a.both_strands, s.ch, s.ch.cidx[s.V], s.al, "--align");
}

// the mappings of every read picked from s.al (the first pass's alignments, or the merged ones)
inline void select(const Args &a, State &s)
{
    const uint64_t R = s.ref.names.size(), C = s.al.alns.size() - 1;
    s.hits.assign(C + 1, kiss_hip_hit{}); // (a read keeps no more hits than it has alignments: one call)
    s.hidx.assign(s.Q + 1, 0);
    s.select_rep = kiss_hip_select_report{};
    check(kiss_hip_fmi_select_host(s.al.alns.data(), s.ch.cidx.data(), s.rd.ridx.data(), s.Q, a.both_strands, R ? s.ref.bounds.data() : nullptr, R,
                                   &a.select_params, s.hits.data(), s.hidx.data(), C, &s.select_rep, a.device),
          "kiss_hip_fmi_select_host");
}

// --sam: the records of the reference, which must add up to the text, and the mappings of every read
inline void load_records(const Args &a, State &s)
{
    s.ref = scan_records(a.fasta);
    if (s.ref.bounds.back() != s.S.size())
        throw std::runtime_error("fmindex_query --sam: the records of " + a.fasta + " have " + std::to_string(s.ref.bounds.back()) +
                                 " bases, the parsed text has " + std::to_string(s.S.size()));
}
inline void select_hits(const Args &a, State &s)
{
    load_records(a, s);
    select(a, s);
}

// --mates: the parameters of the pair call and of the rescue plan.  With --ins-auto the insert size is estimated from the first
// hits of the pairs (the first select call's) and, with enough samples, takes the place of --ins-min / --ins-max / --ins-mean;
// the rescue windows are laid with the values that are used.  One line on stderr says what was found.
inline void insert_size(const Args &a, State &s)
{
    s.pair_params = a.pair_params;
    if (a.ins_auto) {
        kiss_hip_insert_report rep{};
        check(kiss_hip_fmi_insert_host(s.hits.data(), s.hidx.data(), s.Q, s.al.alns.data(), s.select_rep.alignments, &a.insert_params, nullptr, &rep,
                                       a.device),
              "kiss_hip_fmi_insert_host");
        const bool applied = (rep.flags & KISS_HIP_INSERT_OK) != 0;
        if (applied) {
            s.pair_params.ins_min = rep.ins_min;
            s.pair_params.ins_max = rep.ins_max;
            s.pair_params.ins_mean = rep.ins_mean;
        }
        std::cerr << "[insert] pairs=" << rep.P << " samples=" << rep.samples << " used=" << rep.used << " q25=" << rep.q25 << " q50=" << rep.q50
                  << " q75=" << rep.q75 << " mean=" << rep.mean << " sd=" << rep.sd << " ins_min=" << rep.ins_min << " ins_max=" << rep.ins_max
                  << " applied=" << (applied ? 1 : 0) << "\n";
    }
    s.rescue_params = a.rescue_params;
    s.rescue_params.ins_min = s.pair_params.ins_min;
    s.rescue_params.ins_max = s.pair_params.ins_max;
}

// The first pass paired, the pairs that are not proper planned into windows, the windows aligned, their alignments merged
// behind the reads' own (they take the first pass's place in the State), the mappings picked again
inline void rescue_mates(const Args &a, State &s)
{
    const uint64_t Q = s.Q, V = 2 * Q, R = s.ref.names.size(), CA = s.select_rep.alignments, n = s.S.size();
    const uint64_t *bounds = R ? s.ref.bounds.data() : nullptr;
    s.first_alns = CA;
    s.first_pairs.resize(Q / 2 + 1);
    check(kiss_hip_fmi_pair_host(s.hits.data(), s.hidx.data(), Q, s.al.alns.data(), CA, &s.pair_params, s.first_pairs.data(), nullptr, a.device),
          "kiss_hip_fmi_pair_host");
    Chains win;
    win.chains.resize(1);
    win.cidx.assign(V + 1, 0);
    check(sized_call(win.chains, s.plan.chains, [&](uint64_t capacity) {
              return kiss_hip_fmi_rescue_host(s.first_pairs.data(), s.hits.data(), s.hidx.data(), Q, s.al.alns.data(), CA, s.rd.ridx.data(), n, bounds, R,
                                              &s.rescue_params, win.chains.data(), win.cidx.data(), nullptr, capacity, &s.plan, a.device);
          }),
          "kiss_hip_fmi_rescue_host");
    const uint64_t CB = s.plan.chains;
    Alignments wal, mal;
    align(a, s, 1, win, CB, wal, "--rescue");
    const uint64_t C = CA + CB, ops = s.al.oidx[CA] + wal.oidx[CB]; // merged: capacities are known
    mal.alns.resize(C + 1);
    mal.oidx.assign(C + 1, 0);
    mal.cigar.resize(ops + 1);
    std::vector<uint64_t> mcidx(V + 1, 0);
    s.source.resize(C + 1);
    check(kiss_hip_fmi_aln_merge_host(s.al.alns.data(), s.ch.cidx.data(), s.al.cigar.data(), s.al.oidx.data(), wal.alns.data(), win.cidx.data(),
                                      wal.cigar.data(), wal.oidx.data(), V, mal.alns.data(), C, mcidx.data(), s.source.data(), mal.cigar.data(),
                                      mal.oidx.data(), ops, nullptr, a.device),
          "kiss_hip_fmi_aln_merge_host");
    s.al = std::move(mal);
    s.ch.cidx = std::move(mcidx);
    select(a, s);
}

// --md: the MD strings of the hits that the last select picked, written on the device (size then fill)
inline void md_tags(const Args &a, State &s)
{
    const uint64_t H = s.select_rep.hits;
    s.midx.assign(H + 1, 0);
    s.md.resize(1);
    kiss_hip_md_report rep{};
    check(sized_call(s.md, rep.md_bytes, [&](uint64_t capacity) {
              return kiss_hip_fmi_md_host(s.S.data(), s.S.size(), s.rd.reads.data(), s.rd.ridx.data(), s.Q, a.both_strands, s.al.alns.data(),
                                          s.ch.cidx.data(), s.al.cigar.data(), s.al.oidx.data(), s.hits.data(), H, s.md.data(), s.midx.data(), nullptr,
                                          capacity, &rep, a.device);
          }),
          "kiss_hip_fmi_md_host");
    if (rep.bad) throw std::runtime_error("fmindex_query --md: " + std::to_string(rep.bad) + " alignments do not fit their reads");
}

// --mates: the mappings of reads 2 p and 2 p + 1 paired
inline void pair_mates(const Args &a, State &s)
{
    s.pairs.resize(s.Q / 2 + 1);
    check(kiss_hip_fmi_pair_host(s.hits.data(), s.hidx.data(), s.Q, s.al.alns.data(), s.select_rep.alignments, &s.pair_params, s.pairs.data(),
                                 &s.pair_rep, a.device),
          "kiss_hip_fmi_pair_host");
}

// The State as the input of the device writers (include/kiss_hip_sam.h): the names of the reads and of the records go up as byte
// arrays with their spans.  A pair that is bad input: the message of sam_lines.
struct DeviceLinesInput {
    std::vector<uint8_t> names, ref_names;
    std::vector<uint64_t> name_off, ref_name_index;
    std::vector<uint32_t> name_len;
    kiss_hip_sam_input in{};
    DeviceLinesInput(const DeviceLinesInput &) = delete;
    DeviceLinesInput &operator=(const DeviceLinesInput &) = delete;
    DeviceLinesInput(const State &s, bool paired) : name_off(s.Q), ref_name_index(s.ref.names.size() + 1, 0), name_len(s.Q)
    {
        const uint64_t Q = s.Q, R = s.ref.names.size();
        for (uint64_t p = 0; paired && p < Q / 2; p++)
            if (s.pairs[p].flags & KISS_HIP_PAIR_BAD_INPUT)
                throw std::runtime_error("kiss_hip_fmi_pair_host: pair " + std::to_string(s.first / 2 + p) + " is bad input");
        for (uint64_t q = 0; q < Q; q++) {
            name_off[q] = names.size();
            name_len[q] = (uint32_t)s.rd.names[q].size();
            names.insert(names.end(), s.rd.names[q].begin(), s.rd.names[q].end());
        }
        for (uint64_t r = 0; r < R; r++) {
            ref_names.insert(ref_names.end(), s.ref.names[r].begin(), s.ref.names[r].end());
            ref_name_index[r + 1] = ref_names.size();
        }
        names.push_back(0), ref_names.push_back(0); // (no NULL for reads without names)
        static const uint32_t none = 0; // (no NULL for a batch without ops, alignments or hits)
        static const kiss_hip_aln no_aln{};
        static const kiss_hip_hit no_hit{};
        in.reads = s.rd.reads.data(), in.read_index = s.rd.ridx.data(), in.qual = s.rd.has_qual ? s.rd.qual.data() : nullptr;
        in.names = names.data(), in.name_off = name_off.data(), in.name_len = name_len.data();
        in.alns = s.al.alns.empty() ? &no_aln : s.al.alns.data(), in.cigar = s.al.cigar.empty() ? &none : s.al.cigar.data(), in.cigar_index = s.al.oidx.data();
        in.hits = s.hits.empty() ? &no_hit : s.hits.data(), in.hit_index = s.hidx.data();
        in.pairs = paired ? s.pairs.data() : nullptr;
        in.source = s.source.empty() ? nullptr : s.source.data(), in.first_alns = s.first_alns;
        in.md = s.midx.empty() ? nullptr : s.md.data(), in.md_index = s.midx.empty() ? nullptr : s.midx.data();
        in.ref_names = ref_names.data(), in.ref_name_index = ref_name_index.data(), in.bounds = s.ref.bounds.data();
        in.Q = Q, in.C = s.al.oidx.size() - 1, in.R = R;
    }
};

// --sam-writer device: the lines of the State written on the device, in the place of sam_lines.  A pair that is bad input: no
// line of this batch (the device call writes nothing for a batch that has a bad read).
inline void sam_lines_device(StdoutWriter &w, const Args &a, const State &s, bool paired)
{
    const uint64_t Q = s.Q;
    if (!Q) return;
    const DeviceLinesInput d(s, paired);
    std::vector<uint8_t> sam(1);
    std::vector<uint64_t> read_line(Q + 1);
    kiss_hip_sam_report rep{};
    const int rc = sized_call(sam, rep.sam_bytes, [&](uint64_t capacity) {
        return kiss_hip_fmi_sam_host(&d.in, sam.data(), capacity, nullptr, 0, read_line.data(), &rep, a.device);
    });
    if (rc == KISS_HIP_E_INVALID && rep.bad)
        throw std::runtime_error("fmindex_query --sam-writer device: " + std::to_string(rep.bad) + " reads have hits that do not fit them, the first is read " +
                                 std::to_string(s.first + rep.first_bad));
    check(rc, "kiss_hip_fmi_sam_host");
    w.write(); // (what is waiting, the header for one, goes first)
    std::fwrite(sam.data(), 1, rep.sam_bytes, stdout);
}

// --bam FILE: the header (cli_bam.hpp), the records of every batch (kiss_hip_fmi_bam_host) and the end-of-file block, each framed
// as BGZF blocks on the device (kiss_hip_bgzf_host; with --bam-compress kiss_hip_bgzf_deflate_host, which compresses them) and
// written as it comes.  FILE is opened before a read is mapped.
// --bam-sort: the header and the unframed records of every batch are kept (cli_bam_sort.hpp) until close(), which sorts the records
// of the whole file on the device (kiss_hip_bam_sort_host) and only then frames and writes the header, with SO:coordinate, the
// records and the end-of-file block.
// --bam-index: the sort also gives the CSR of the sorted records and the framing of the records the offsets of its blocks
// (cli_bam_index.hpp); kiss_hip_bai_host builds the index from both and the framed header's length, and FILE.bai is written
// behind FILE.
// --bam-markdup: directly before the sort, kiss_hip_bam_markdup_host sets FLAG 0x400 in the kept records of the duplicate
// templates, in place: the records of a read are still together there.
struct BamOut {
    std::string path;
    std::FILE *file = nullptr;
    int device = 0;
    bool compress = false, sort = false, index = false, markdup = false;
    uint32_t markdup_min_qual = KISS_HIP_MARKDUP_MIN_QUAL_DEFAULT;
    uint64_t records = 0, bytes = 0;
    BamSortRecords kept;     // --bam-sort: the records so far
    std::string kept_header; // ... and the header, unframed
    uint32_t n_ref = 0;
    BamOut() = default;
    BamOut(const BamOut &) = delete;
    BamOut &operator=(const BamOut &) = delete;
    ~BamOut()
    {
        if (file && file != stdout) std::fclose(file);
    }
    bool on() const { return file != nullptr; }
    void open(const Args &a)
    {
        path = a.bam, device = a.device, compress = a.bam_compress, sort = a.bam_sort, index = a.bam_index;
        markdup = a.bam_markdup, markdup_min_qual = a.bam_markdup_min_qual;
        file = path == "-" ? stdout : std::fopen(path.c_str(), "wb");
        if (!file) throw std::runtime_error("cannot open " + path);
    }
    // data[0, n) as BGZF blocks; eof: the end-of-file block behind them; keep: what the index needs of the framing, or null; hold:
    // the blocks go behind what it holds, not to FILE (they count as written: `bytes` is where they will stand), or null
    void framed(const uint8_t *data, uint64_t n, int eof, BamIndexFrame *keep = nullptr, std::vector<uint8_t> *hold = nullptr)
    {
        const uint64_t total = n + (uint64_t)KISS_HIP_BGZF_OVERHEAD * ((n + KISS_HIP_BGZF_BLOCK_DEFAULT - 1) / KISS_HIP_BGZF_BLOCK_DEFAULT) +
                               (eof ? KISS_HIP_BGZF_EOF_BYTES : 0u);
        std::vector<uint8_t> out(total + 1);
        uint64_t out_bytes = 0;
        if (compress) { // (total is the worst case: every block stored)
            kiss_hip_bgzf_deflate_report rep{};
            const uint64_t entries = keep ? keep->room(n, KISS_HIP_BGZF_BLOCK_DEFAULT) : 0;
            check(kiss_hip_bgzf_deflate_host(n ? data : nullptr, n, 0, eof, out.data(), total, keep ? keep->block_index.data() : nullptr, entries, &rep, device),
                  "kiss_hip_bgzf_deflate_host");
            out_bytes = rep.out_bytes;
            if (keep) keep->check(out_bytes);
        } else {
            kiss_hip_bgzf_report rep{};
            check(kiss_hip_bgzf_host(n ? data : nullptr, n, 0, eof, out.data(), total, &rep, device), "kiss_hip_bgzf_host");
            out_bytes = rep.out_bytes;
        }
        if (hold) hold->insert(hold->end(), out.begin(), out.begin() + (std::ptrdiff_t)out_bytes);
        else if (std::fwrite(out.data(), 1, out_bytes, file) != out_bytes) throw std::runtime_error("cannot write " + path);
        bytes += out_bytes;
    }
    void header(const RefRecords &ref, const char *version)
    {
        std::string text;
        sam_header(text, ref, version);
        if (sort) {
            kept_header = bam_header(sam_header_coordinate(text), ref.names, ref.bounds);
            n_ref = (uint32_t)ref.names.size();
            return;
        }
        const std::string h = bam_header(text, ref.names, ref.bounds);
        framed(reinterpret_cast<const uint8_t *>(h.data()), h.size(), 0);
    }
    // the records of the State, in the place of its lines
    void add(const State &s, bool paired)
    {
        if (!s.Q) return;
        const DeviceLinesInput d(s, paired);
        std::vector<uint8_t> bam(1);
        std::vector<uint64_t> read_rec(s.Q + 1), rec_index(1);
        kiss_hip_bam_report rep{};
        const int rc = sized_call(bam, rep.bam_bytes, [&](uint64_t capacity) {
            if (!sort) return kiss_hip_fmi_bam_host(&d.in, bam.data(), capacity, nullptr, 0, read_rec.data(), &rep, device);
            if (rec_index.size() < rep.records + 1) rec_index.resize(rep.records + 1); // (the sizing call has left the count)
            return kiss_hip_fmi_bam_host(&d.in, bam.data(), capacity, rec_index.data(), rec_index.size() - 1, read_rec.data(), &rep, device);
        });
        if (rc == KISS_HIP_E_INVALID && rep.bad)
            throw std::runtime_error("fmindex_query --bam: " + std::to_string(rep.bad) + " reads cannot be written as BAM (kiss --help-bam), the first is read " +
                                     std::to_string(s.first + rep.first_bad));
        check(rc, "kiss_hip_fmi_bam_host");
        if (sort) kept.add(bam.data(), rep.bam_bytes, rec_index.data(), rep.records);
        else framed(bam.data(), rep.bam_bytes, 0);
        records += rep.records;
    }
    // --bam-markdup: the kept records of the whole file, in the order they were written, marked in place
    void marked()
    {
        const uint64_t n = kept.bytes.size();
        kiss_hip_markdup_report rep{};
        const int rc = kiss_hip_bam_markdup_host(n ? kept.bytes.data() : nullptr, n, kept.index.data(), kept.records(), n_ref, markdup_min_qual, nullptr,
                                                 &rep, device);
        if (rc == KISS_HIP_E_INVALID && rep.bad)
            throw std::runtime_error("fmindex_query --bam-markdup: " + std::to_string(rep.bad) + " records cannot be read, the first is record " +
                                     std::to_string(rep.first_bad));
        check(rc, "kiss_hip_bam_markdup_host");
        std::fprintf(stderr, "[info] bam markdup: templates: %llu, duplicate pairs: %llu, duplicate fragments: %llu, duplicate records: %llu\n",
                     (ull)rep.templates, (ull)rep.dup_pairs, (ull)rep.dup_fragments, (ull)rep.dup_records);
    }
    // --bam-sort: the whole file, once
    void sorted()
    {
        if (markdup) marked();
        const uint64_t n = kept.bytes.size();
        std::vector<uint8_t> out(n + 1);
        std::vector<uint64_t> sorted_index(index ? kept.records() + 1 : 0);
        kiss_hip_bam_sort_report rep{};
        const int rc = kiss_hip_bam_sort_host(n ? kept.bytes.data() : nullptr, n, kept.index.data(), kept.records(), n_ref, out.data(), n,
                                              index ? sorted_index.data() : nullptr, nullptr, &rep, device);
        if (rc == KISS_HIP_E_INVALID && rep.bad)
            throw std::runtime_error("fmindex_query --bam-sort: " + std::to_string(rep.bad) + " records cannot be sorted, the first is record " +
                                     std::to_string(rep.first_bad));
        check(rc, "kiss_hip_bam_sort_host");
        BamSortRecords().bytes.swap(kept.bytes); // (the unsorted copy is not needed any more)
        std::fprintf(stderr, "[info] bam sort: records: %llu, unplaced: %llu, longest record: %llu\n", (ull)rep.records, (ull)rep.unplaced, (ull)rep.longest);
        if (!index) {
            framed(reinterpret_cast<const uint8_t *>(kept_header.data()), kept_header.size(), 0);
            framed(out.data(), n, 0);
            return;
        }
        // with the index nothing reaches FILE before FILE.bai is complete in memory: an index that refuses the records (an end
        // beyond 2^29, say) ends the run with FILE empty, not cut off behind its last record block
        std::vector<uint8_t> blocks;
        framed(reinterpret_cast<const uint8_t *>(kept_header.data()), kept_header.size(), 0, nullptr, &blocks);
        BamIndexFrame frame;
        frame.file_base = bytes; // (nothing but the framed header stands in front of the record blocks)
        framed(out.data(), n, 0, &frame, &blocks);
        indexed(out.data(), n, sorted_index, frame);
        if (std::fwrite(blocks.data(), 1, blocks.size(), file) != blocks.size()) throw std::runtime_error("cannot write " + path);
    }
    // --bam-index: the bytes of FILE.bai, kept until FILE is complete
    std::vector<uint8_t> bai;
    void indexed(const uint8_t *bam, uint64_t n, const std::vector<uint64_t> &rec_index, const BamIndexFrame &frame)
    {
        kiss_hip_bai_report rep{};
        bai.assign(1, 0);
        const int rc = sized_call(bai, rep.bai_bytes, [&](uint64_t capacity) {
            return kiss_hip_bai_host(n ? bam : nullptr, n, rec_index.data(), rec_index.size() - 1, n_ref, KISS_HIP_BGZF_BLOCK_DEFAULT, frame.offsets(),
                                     frame.file_base, bai.data(), capacity, &rep, device);
        });
        if (rc == KISS_HIP_E_INVALID && rep.bad)
            throw std::runtime_error("fmindex_query --bam-index: " + std::to_string(rep.bad) + " records cannot be indexed (kiss --help-bam), the first is record " +
                                     std::to_string(rep.first_bad));
        check(rc, "kiss_hip_bai_host");
        bai.resize(rep.bai_bytes);
        std::fprintf(stderr, "[info] bam index: bytes: %llu, bins: %llu, chunks: %llu, windows: %llu, no_coor: %llu\n", (ull)rep.bai_bytes, (ull)rep.bins,
                     (ull)rep.chunks, (ull)rep.windows, (ull)rep.no_coor);
    }
    void write_index()
    {
        const std::string to = bam_index_path(path);
        std::FILE *f = std::fopen(to.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot open " + to);
        const bool ok = std::fwrite(bai.data(), 1, bai.size(), f) == bai.size();
        if (std::fclose(f) != 0 || !ok) throw std::runtime_error("cannot write " + to);
    }
    void close()
    {
        if (sort) sorted();
        framed(nullptr, 0, 1);
        if (std::fflush(file) != 0) throw std::runtime_error("cannot write " + path);
        if (index) write_index(); // (FILE.bai after FILE)
        std::fprintf(stderr, "[info] bam: records: %llu, bytes: %llu\n", (ull)records, (ull)bytes);
    }
};

// --pileup FILE: ONE device array of 8 planes of n u32 (32 n bytes) to which every batch adds -- kiss_hip_fmi_pileup_host with
// counts_on_device, accumulate from the second call on --, fetched once behind the last batch and written as lines
// (cli_pileup.hpp).  The array is allocated and FILE opened before a read is mapped.
struct PileupSums {
    std::string path;
    std::FILE *file = nullptr;
    uint32_t *d = nullptr;
    uint64_t n = 0, calls = 0;
    kiss_hip_pileup_report total{};
    PileupSums() = default;
    PileupSums(const PileupSums &) = delete;
    PileupSums &operator=(const PileupSums &) = delete;
    ~PileupSums()
    {
        if (d) kiss_hip_free_dev(d);
        if (file) std::fclose(file);
    }
    bool on() const { return file != nullptr; }
    // (behind load_text: its context has made a.device the current one)
    void open(const Args &a, uint64_t bases)
    {
        path = a.pileup, n = bases;
        void *p = nullptr;
        if (n && kiss_hip_alloc_dev(&p, 32 * n) != KISS_HIP_OK)
            throw std::runtime_error("fmindex_query --pileup: cannot allocate the " + std::to_string(32 * n) + " bytes of the counts on the device (32 per base of the text)");
        d = static_cast<uint32_t *>(p);
        file = std::fopen(path.c_str(), "wb");
        if (!file) throw std::runtime_error("cannot open " + path);
    }
    // the hits of the last select call (paired: the pairs of the last pair call) added
    void add(const Args &a, const State &s, bool paired)
    {
        kiss_hip_pileup_report rep{};
        check(kiss_hip_fmi_pileup_host(s.S.data(), s.S.size(), s.rd.reads.data(), s.rd.ridx.data(), s.Q, a.both_strands, s.al.alns.data(),
                                       s.ch.cidx.data(), s.al.cigar.data(), s.al.oidx.data(), s.hits.data(), s.select_rep.hits,
                                       paired ? s.pairs.data() : nullptr, paired ? s.Q / 2 : 0, &a.pileup_params, 0, n, d, 1, calls ? 1 : 0, &rep,
                                       a.device),
              "kiss_hip_fmi_pileup_host");
        calls++;
        total.items += rep.items, total.bad += rep.bad, total.filtered += rep.filtered, total.unmapped += rep.unmapped, total.counted += rep.counted;
        total.columns += rep.columns, total.alt_columns += rep.alt_columns, total.deleted_bases += rep.deleted_bases;
        total.insertions += rep.insertions, total.clipped += rep.clipped;
    }
    // the sums fetched once and written; S and ref: the text and its records
    void write(const std::vector<uint8_t> &S, const RefRecords &ref)
    {
        std::vector<uint32_t> planes(8 * n + 1, 0);
        if (n && calls) check(kiss_hip_copy_to_host(planes.data(), d, 32 * n), "kiss_hip_copy_to_host");
        write_pileup(file, path, planes.data(), n, S.data(), ref.names, ref.bounds);
        std::fprintf(stderr, "[info] pileup: items: %llu, counted: %llu, filtered: %llu, unmapped: %llu, bad: %llu, columns: %llu, differing: %llu, "
                             "deleted bases: %llu, insertions: %llu\n",
                     (ull)total.items, (ull)total.counted, (ull)total.filtered, (ull)total.unmapped, (ull)total.bad, (ull)total.columns,
                     (ull)total.alt_columns, (ull)total.deleted_bases, (ull)total.insertions);
    }
};

// --batch-reads N: the text and the records of the reference loaded once, the header printed once; then every batch of N reads,
// or of N pairs, cut from the files by a ChunkReader, gives a State, the stages above and its lines.  The stages are the _host
// entries: each uploads the index or the text once more per batch (DESIGN.md 4.20 says what that costs).  --ins-auto: estimated
// from batch 0, whose values serve every later batch.  An error of a later batch comes behind the lines of the earlier ones.
inline int map_reads_in_batches(const Args &a, const kiss_hip_fmi_view_ex &index)
{
    const auto part = [&a](const uint8_t *raw, uint64_t bytes, int format, int final, uint64_t max_records, uint8_t *codes, uint8_t *qual,
                           uint64_t bases_capacity, uint64_t *read_index, uint64_t *name_off, uint32_t *name_len, uint64_t reads_capacity,
                           kiss_hip_reads_part_report *rep) {
        const int rc = kiss_hip_reads_parse_part_host(raw, bytes, format, final, max_records, codes, qual, bases_capacity, read_index, name_off,
                                                      name_len, reads_capacity, rep, a.device);
        if (rc != KISS_HIP_E_INVALID) check(rc, "kiss_hip_reads_parse_part_host");
        return rc;
    };
    typedef ChunkReader<decltype(part)> Reader;
    const int wanted = a.reads_format == "lines" ? KISS_HIP_READS_LINES : a.reads_format == "fastq" ? KISS_HIP_READS_FASTQ : KISS_HIP_READS_AUTO;
    const bool paired = !a.mates.empty();
    std::vector<Reader> files;
    files.reserve(2);
    files.emplace_back(a.seeds, wanted, a.batch_chunk, true, part);
    if (paired) files.emplace_back(a.mates, wanted, a.batch_chunk, true, part);
    State keep; // the text and the records pass from batch to batch
    load_text(a, keep);
    load_records(a, keep);
    PileupSums pile;
    if (!a.pileup.empty()) pile.open(a, keep.S.size());
    BamOut bam;
    if (!a.bam.empty()) bam.open(a);
    kiss_hip_pair_params pair_params{};
    kiss_hip_rescue_params rescue_params{};
    StdoutWriter w;
    uint64_t batches = 0, reads = 0, mapped = 0;
    for (;; batches++) {
        uint64_t K = files[0].ready(a.batch_reads);
        if (paired) {
            const uint64_t K2 = files[1].ready(a.batch_reads);
            if (!K != !K2) {
                const Reader &shorter = files[K ? 1 : 0];
                throw std::runtime_error("fmindex_query --mates: " + shorter.path() + " ends after " + std::to_string(shorter.first()) +
                                         " reads, " + files[K ? 0 : 1].path() + " has more: a pair has one of each");
            }
            K = std::min(K, K2);
        }
        if (!K) break;
        State s;
        s.index = index;
        s.S = std::move(keep.S);
        s.ref = std::move(keep.ref);
        s.first = (paired ? 2 : 1) * files[0].first();
        s.rd = files[0].take(K);
        if (paired) {
            ReadFile first = std::move(s.rd), second = files[1].take(K);
            if (files[0].format() != files[1].format()) refuse_formats(a);
            s.rd = interleave_mates(a, first, second, files[0].format());
        }
        s.Q = s.rd.ridx.size() - 1;
        s.V = a.both_strands ? 2 * s.Q : s.Q;
        find_seeds(a, s);
        chain_seeds(a, s);
        align(a, s, a.both_strands, s.ch, s.ch.cidx[s.V], s.al, "--align");
        select(a, s);
        if (paired && !batches) insert_size(a, s), pair_params = s.pair_params, rescue_params = s.rescue_params;
        if (paired) s.pair_params = pair_params, s.rescue_params = rescue_params;
        if (a.rescue) rescue_mates(a, s);
        if (paired) pair_mates(a, s);
        if (a.md) md_tags(a, s);
        if (pile.on()) pile.add(a, s, paired);
        if (bam.on()) {
            if (!batches) bam.header(s.ref, VERSION);
            bam.add(s, paired);
        } else {
            if (!batches) sam_header(w.out, s.ref, VERSION);
            if (a.sam_writer == "device") sam_lines_device(w, a, s, paired);
            else sam_lines(w, s, paired);
            w.finish(); // (on stdout before the next batch can fail)
        }
        if (a.verbose) sam_info(s, paired, a.rescue);
        reads += s.Q, mapped += s.select_rep.mapped;
        keep.S = std::move(s.S);
        keep.ref = std::move(s.ref);
    }
    if (!batches && bam.on()) bam.header(keep.ref, VERSION);
    if (!batches && !bam.on()) sam_header(w.out, keep.ref, VERSION), w.finish();
    if (bam.on()) bam.close();
    if (pile.on()) pile.write(keep.S, keep.ref);
    std::fprintf(stderr, "[info] batches: %llu, reads: %llu, mapped: %llu\n", (ull)batches, (ull)reads, (ull)mapped);
    return 0;
}

// fmindex_query --seeds: `index` is the view of the .fmi of a.fasta
inline int map_reads(const Args &a, const kiss_hip_fmi_view_ex &index)
{
    if (a.batch_reads) return map_reads_in_batches(a, index);
    State s;
    s.index = index;
    PileupSums pile;
    if (!a.pileup.empty()) load_text(a, s), pile.open(a, s.S.size()); // (before a read is mapped)
    BamOut bam;
    if (!a.bam.empty()) bam.open(a);
    load_reads(a, s);
    find_seeds(a, s);
    if (!a.chain) return print_seeds(s, a.both_strands);
    chain_seeds(a, s);
    if (!a.align) return print_chains(s, a.both_strands);
    if (pile.on()) align(a, s, a.both_strands, s.ch, s.ch.cidx[s.V], s.al, "--align");
    else align_chains(a, s);
    if (!a.sam) return print_alignments(s, a.both_strands);
    select_hits(a, s);
    if (!a.mates.empty()) insert_size(a, s);
    if (a.rescue) rescue_mates(a, s);
    if (!a.mates.empty()) pair_mates(a, s);
    if (a.md) md_tags(a, s);
    if (pile.on()) pile.add(a, s, !a.mates.empty());
    if (bam.on()) {
        bam.header(s.ref, VERSION);
        bam.add(s, !a.mates.empty());
        bam.close();
        sam_info(s, !a.mates.empty(), a.rescue);
    } else if (a.sam_writer != "device") {
        print_sam(s, !a.mates.empty(), a.rescue, VERSION);
    } else {
        StdoutWriter w;
        sam_header(w.out, s.ref, VERSION);
        sam_lines_device(w, a, s, !a.mates.empty());
        w.finish();
        sam_info(s, !a.mates.empty(), a.rescue);
    }
    if (pile.on()) pile.write(s.S, s.ref);
    return 0;
}

} // namespace kiss_cli
