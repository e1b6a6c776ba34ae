// cli_format.hpp -- what `kiss fmindex_query --seeds` reads, holds and prints, free of the library: the two file parsers (the
// reads, the records of the reference), the State that the stages of cli_reads.hpp fill, and a printer for every place the
// pipeline can end at: the lines of --seeds / --chain / --align and SAM (one line function for every hit and every unmapped
// read or mate, single-end and paired on top of it), each with its [info] line.  Needs kiss_hip.h for the record types and
// flag constants only and calls no kiss_hip_* function, so it is tested without a device (tests/test_cli_format.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/kiss_hip.h"

namespace kiss_cli {

// stdout through a string: flushed when a caller says a good place has come and 1 MiB has gathered, and at the end
struct StdoutWriter {
    std::string out;
    void write() { std::fwrite(out.data(), 1, out.size(), stdout); out.clear(); }
    void flush_if_full() { if (out.size() > (1u << 20)) write(); }
    void finish() { write(); std::fflush(stdout); }
};

// The records of the reference file, scanned on the host under the parse rules of fasta.hip: the file is FASTA iff its first
// byte is '>'; a line that begins with '>' is a header unless the line in front of it was one (the line after a header is
// always sequence); every byte of a sequence line except '\n' is a base.  A plain-text file is one record named after the
// file.  Records without bases are left out (SAM has no LN:0, and the record starts must ascend strictly).
struct RefRecords { std::vector<std::string> names; std::vector<uint64_t> bounds{0}; };
inline RefRecords scan_records(const std::string &path) // (streamed: a file may be one line of gigabytes)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    RefRecords r;
    std::string name = path.substr(path.find_last_of('/') == std::string::npos ? 0 : path.find_last_of('/') + 1);
    uint64_t len = 0;
    const auto close = [&]() {
        if (len) {
            r.names.push_back(name);
            r.bounds.push_back(r.bounds.back() + len);
        }
        len = 0;
    };
    std::vector<char> buf(1 << 20);
    bool first = true, fasta = false, line_start = true, header = false, prev_header = false, in_name = false;
    while (in) {
        in.read(buf.data(), (std::streamsize)buf.size());
        for (std::streamsize i = 0; i < in.gcount(); i++) {
            const char c = buf[(size_t)i];
            if (first) fasta = c == '>';
            first = false;
            if (line_start) { // a record begins with a header line: its name is the word after '>'
                header = in_name = fasta && c == '>' && !prev_header;
                if (header) close(), name.clear();
            }
            if (c == '\n') prev_header = header;
            else if (!header) len++;
            else if (!line_start && in_name && c != ' ' && c != '\t' && c != '\r') name += c;
            else if (!line_start) in_name = false;
            line_start = c == '\n';
        }
    }
    close();
    return r;
}

// One file of reads, one per line ('\r' before the '\n' dropped; empty lines and lines that start with '>' are no reads): the
// codes of the reads one after the other (ACGTacgt -> 0..3, every other letter 4, no base -- in the text it is 0), where they
// start, and with_names their names: the word after '>' on the line directly in front of a read, else its number
struct ReadFile {
    std::vector<uint8_t> reads;
    std::vector<uint64_t> ridx{0};
    std::vector<std::string> names;
    bool has_qual = false;     // the reads came from FASTQ (cli_reads.hpp: load_reads; read_file below gives none):
    std::vector<uint8_t> qual; // the quality byte of every entry of reads
};
inline ReadFile read_file(const std::string &path, bool with_names)
{
    std::ifstream in(path);
    if (!in) throw std::runtime_error("cannot open " + path);
    ReadFile f;
    std::string line, pending;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.empty() || line[0] == '>') {
            if (with_names) {
                const size_t ws = line.find_first_of(" \t", 1);
                pending = line.empty() ? std::string() : line.substr(1, ws == std::string::npos ? std::string::npos : ws - 1);
            }
            continue;
        }
        if (with_names) f.names.push_back(pending.empty() ? std::to_string(f.ridx.size() - 1) : pending);
        pending.clear();
        for (unsigned char c : line) {
            uint8_t code = 4; // no base
            switch (c) {
            case 'A': case 'a': code = 0; break;
            case 'C': case 'c': code = 1; break;
            case 'G': case 'g': code = 2; break;
            case 'T': case 't': code = 3; break;
            default: break;
            }
            f.reads.push_back(code);
        }
        f.ridx.push_back(f.reads.size());
    }
    return f;
}

// the CIGAR of an alignment of a read of L bases, SAM style: the ops between the soft clips of what did not align
inline void cigar_with_clips(std::string &out, const kiss_hip_aln &k, const uint32_t *ops, uint64_t n_ops, uint64_t L)
{
    if (k.rbeg) out += std::to_string(k.rbeg) + 'S';
    for (uint64_t x = 0; x < n_ops; x++) out += std::to_string(ops[x] >> 4) + "MID"[ops[x] & 15u];
    if (L > k.rend) out += std::to_string(L - k.rend) + 'S';
}

// the letters of read q (N: no base), or of its reverse complement
inline std::string read_letters(const std::vector<uint8_t> &reads, const std::vector<uint64_t> &ridx, uint64_t q, bool reverse)
{
    const uint64_t L = ridx[q + 1] - ridx[q];
    std::string s(L, 'N');
    for (uint64_t j = 0; j < L; j++) {
        const uint8_t c = reads[ridx[q] + (reverse ? L - 1 - j : j)];
        if (c <= 3) s[j] = "ACGT"[reverse ? 3 - c : c];
    }
    return s;
}

// QUAL of read q: its quality string as the file has it, reversed (not complemented) where SEQ is; * for a file without qualities
inline std::string read_qual(const ReadFile &rd, uint64_t q, bool reverse)
{
    if (!rd.has_qual) return "*";
    const uint64_t L = rd.ridx[q + 1] - rd.ridx[q];
    std::string s(L, '!');
    for (uint64_t j = 0; j < L; j++) s[j] = (char)rd.qual[rd.ridx[q] + (reverse ? L - 1 - j : j)];
    return s;
}

// the names of Q reads from their spans in the bytes of the file; the number of the read where the span is empty (as read_file)
inline std::vector<std::string> names_from_spans(const std::vector<uint8_t> &raw, const std::vector<uint64_t> &off, const std::vector<uint32_t> &len,
                                                 uint64_t Q)
{
    std::vector<std::string> names;
    for (uint64_t q = 0; q < Q; q++)
        names.push_back(len[q] ? std::string((const char *)raw.data() + off[q], len[q]) : std::to_string(q));
    return names;
}

// FASTQ mates: a name that ends in /1 or /2 loses those two bytes, so that both mates of a pair carry one QNAME
inline void strip_mate_suffix(std::string &name)
{
    const size_t n = name.size();
    if (n >= 2 && name[n - 2] == '/' && (name[n - 1] == '1' || name[n - 1] == '2')) name.resize(n - 2);
}

// What the stages make, in their order.  Alignment c: al.alns[c] and the ops al.oidx[c] .. al.oidx[c + 1]; the hits of read q:
// hits[hidx[q]] .. hits[hidx[q + 1]]; reads 2 p and 2 p + 1 are the mates of pair p.
struct Chains { std::vector<kiss_hip_chain> chains; std::vector<uint64_t> cidx; }; // (or the windows of --rescue) per virtual read
struct Alignments { std::vector<kiss_hip_aln> alns; std::vector<uint32_t> cigar; std::vector<uint64_t> oidx; kiss_hip_align_report rep{}; };
struct State {
    kiss_hip_fmi_view_ex index{}; // (of the caller's .fmi)
    ReadFile rd;                  // load_reads: Q reads, V virtual reads: with --both-strands two of each, strand + then -
    uint64_t Q = 0, V = 0;
    uint64_t first = 0;           // --batch-reads: the number in the file of read 0 of this batch (mates: of the interleaved reads)
    std::vector<kiss_hip_fmi_seed> seeds; // find_seeds
    std::vector<uint64_t> sidx, pidx;
    std::vector<uint32_t> pos;
    kiss_hip_fmi_seed_report seed_rep{};
    Chains ch; // chain_seeds (after --rescue cidx is the merged alignments')
    kiss_hip_chain_report chain_rep{};
    std::vector<uint8_t> S; // align_chains: the text
    Alignments al;          // (after --rescue the merged ones)
    RefRecords ref;         // select_hits
    std::vector<kiss_hip_hit> hits;
    std::vector<uint64_t> hidx;
    kiss_hip_select_report select_rep{};
    // rescue_mates: alignment c came from a window iff source[c] >= first_alns; the first pass's pairs; the plan's report
    std::vector<uint32_t> source;
    uint64_t first_alns = 0;
    std::vector<kiss_hip_pair> first_pairs;
    kiss_hip_rescue_report plan{};
    std::vector<kiss_hip_pair> pairs; // pair_mates
    // md_tags (--md): the MD string of hit h is md[midx[h]] .. md[midx[h + 1]]; midx empty: no MD tags
    std::vector<uint8_t> md;
    std::vector<uint64_t> midx;
    kiss_hip_pair_report pair_rep{};
    // the pair and rescue parameters that are used: the command line's, or with --ins-auto the estimated insert in them
    kiss_hip_pair_params pair_params{};
    kiss_hip_rescue_params rescue_params{};
};

// ---- the printers: stdout, then the [info] line on stderr -------------------------------------------------------------------
typedef unsigned long long ull;
// line(out, read, i) after "read strand " for every entry i of idx[v] .. idx[v + 1] of every virtual read v
template <class Line> void print_per_virtual_read(const State &s, bool both_strands, const std::vector<uint64_t> &idx, Line line)
{
    StdoutWriter w;
    for (uint64_t vr = 0; vr < s.V; vr++) {
        for (uint64_t i = idx[vr]; i < idx[vr + 1]; i++) {
            const uint64_t q = both_strands ? vr / 2 : vr;
            w.out += std::to_string(q) + ' ' + (both_strands && (vr & 1) ? '-' : '+') + ' ';
            line(w.out, q, i);
            w.out += '\n';
        }
        w.flush_if_full();
    }
    w.finish();
}

// read strand start len count pos...
inline int print_seeds(const State &s, bool both_strands)
{
    print_per_virtual_read(s, both_strands, s.sidx, [&](std::string &out, uint64_t, uint64_t i) {
        out += std::to_string(s.seeds[i].start) + ' ' + std::to_string(s.seeds[i].len) + ' ' + std::to_string(s.seeds[i].sa_end - s.seeds[i].sa_beg);
        for (uint64_t x = s.pidx[i]; x < s.pidx[i + 1]; x++) out += ' ' + std::to_string(s.pos[x]);
    });
    std::fprintf(stderr, "[info] reads: %llu, seeds: %llu, located seeds: %llu, positions: %llu\n", (ull)s.Q, (ull)s.seed_rep.seeds,
                 (ull)s.seed_rep.located_seeds, (ull)s.seed_rep.positions);
    return 0;
}

// read strand score anchors rbeg rend tbeg tend
inline int print_chains(const State &s, bool both_strands)
{
    print_per_virtual_read(s, both_strands, s.ch.cidx, [&](std::string &out, uint64_t, uint64_t c) {
        const kiss_hip_chain &k = s.ch.chains[c];
        out += std::to_string(k.score) + ' ' + std::to_string(k.anchors) + ' ' + std::to_string(k.rbeg) + ' ' + std::to_string(k.rend) + ' ' +
               std::to_string(k.tbeg) + ' ' + std::to_string(k.tend);
    });
    std::fprintf(stderr, "[info] virtual reads: %llu, anchors: %llu, chains: %llu, best score: %u\n", (ull)s.V, (ull)s.chain_rep.anchors,
                 (ull)s.chain_rep.chains, s.chain_rep.best_score);
    return 0;
}

// read strand score rbeg rend tbeg tend nm cigar (* when nothing aligned)
inline int print_alignments(const State &s, bool both_strands)
{
    print_per_virtual_read(s, both_strands, s.ch.cidx, [&](std::string &out, uint64_t q, uint64_t c) {
        const kiss_hip_aln &k = s.al.alns[c];
        out += std::to_string(k.score) + ' ' + std::to_string(k.rbeg) + ' ' + std::to_string(k.rend) + ' ' + std::to_string(k.tbeg) + ' ' +
               std::to_string(k.tend) + ' ' + std::to_string(k.mismatches + k.ins + k.del) + ' ';
        if (s.al.oidx[c + 1] == s.al.oidx[c]) out += '*';
        else cigar_with_clips(out, k, s.al.cigar.data() + s.al.oidx[c], s.al.oidx[c + 1] - s.al.oidx[c], s.rd.ridx[q + 1] - s.rd.ridx[q]);
    });
    std::fprintf(stderr, "[info] virtual reads: %llu, chains: %llu, aligned: %llu, band too wide: %llu, best score: %u\n", (ull)s.V,
                 (ull)s.al.rep.chains, (ull)s.al.rep.aligned, (ull)s.al.rep.too_wide, s.al.rep.best_score);
    return 0;
}

// ---- SAM --------------------------------------------------------------------------------------------------------------
// what a mate adds to a line; as it stands, the line of a read on its own
struct MateFields {
    unsigned flag = 0;                  // bits ORed into FLAG
    bool chosen = false;                // the hit the pair chose: written without the hit's own 256 / 2048
    const std::string *rnext = nullptr; // the record RNEXT names ("=" where that is the line's own); nullptr: *
    uint64_t pnext = 0;
    long long tlen = 0;
    long mapq = -1, mate_score = -1;      // >= 0: MAPQ instead of the hit's; YS:i:
    bool proper = false, rescued = false; // YT:Z:CP; YR:i:1
};

// The one SAM line of hit t of read q, or with t == nullptr of a read that did not map (FLAG 4; a mate lies where rnext / pnext
// say its partner does).  POS is 1-based in the record; SEQ is reversed where the hit is, and so is QUAL (the qualities of a FASTQ
// read; * otherwise); the tags are NM, MD (--md), AS, XS (heads only), then YS, YT, YR.  Without records (R == 0) RNAME is *.
inline void sam_line(std::string &out, const State &m, uint64_t q, const kiss_hip_hit *t, const MateFields &f)
{
    const uint64_t R = m.ref.names.size(), L = m.rd.ridx[q + 1] - m.rd.ridx[q];
    if (!t) {
        out += m.rd.names[q] + '\t' + std::to_string(f.flag | 4u) + '\t' + (f.rnext ? *f.rnext : "*") + '\t' + std::to_string(f.pnext) + "\t0\t*\t" +
               (f.rnext ? "=" : "*") + '\t' + std::to_string(f.pnext) + "\t0\t" + read_letters(m.rd.reads, m.rd.ridx, q, false) + '\t' +
               read_qual(m.rd, q, false) + '\n';
        return;
    }
    const kiss_hip_aln &k = m.al.alns[t->aln];
    const bool reverse = (t->flags & KISS_HIP_HIT_REVERSE) != 0, head = !(t->flags & KISS_HIP_HIT_SECONDARY);
    unsigned flag = f.flag | (reverse ? 16u : 0u);
    if (!f.chosen) flag |= (t->flags & KISS_HIP_HIT_SECONDARY ? 256u : 0u) | (t->flags & KISS_HIP_HIT_SUPPLEMENTARY ? 2048u : 0u);
    const std::string name = R ? m.ref.names[t->ref] : std::string("*");
    out += m.rd.names[q] + '\t' + std::to_string(flag) + '\t' + name + '\t' + std::to_string((uint64_t)k.tbeg - (R ? m.ref.bounds[t->ref] : 0) + 1) + '\t' +
           std::to_string(f.mapq >= 0 ? (uint32_t)f.mapq : t->mapq) + '\t';
    cigar_with_clips(out, k, m.al.cigar.data() + m.al.oidx[t->aln], m.al.oidx[t->aln + 1] - m.al.oidx[t->aln], L);
    out += '\t' + (!f.rnext ? std::string("*") : name == *f.rnext ? std::string("=") : *f.rnext) + '\t' + std::to_string(f.pnext) + '\t' +
           std::to_string(f.tlen) + '\t' + read_letters(m.rd.reads, m.rd.ridx, q, reverse) + '\t' + read_qual(m.rd, q, reverse) +
           "\tNM:i:" + std::to_string(k.mismatches + k.ins + k.del);
    if (!m.midx.empty()) {
        const uint64_t h = (uint64_t)(t - m.hits.data());
        out += "\tMD:Z:";
        out.append(reinterpret_cast<const char *>(m.md.data()) + m.midx[h], m.midx[h + 1] - m.midx[h]);
    }
    out += "\tAS:i:" + std::to_string(t->score);
    if (head) out += "\tXS:i:" + std::to_string(t->sub);
    if (f.mate_score >= 0) out += "\tYS:i:" + std::to_string(f.mate_score);
    if (f.proper) out += "\tYT:Z:CP";
    if (f.rescued) out += "\tYR:i:1";
    out += '\n';
}

// a read on its own: one line per hit in hit order, or the one line of a read without hits
inline void sam_read_lines(std::string &out, const State &m, uint64_t q)
{
    if (m.hidx[q + 1] == m.hidx[q]) sam_line(out, m, q, nullptr, MateFields());
    for (uint64_t h = m.hidx[q]; h < m.hidx[q + 1]; h++) sam_line(out, m, q, &m.hits[h], MateFields());
}

// Reads 2 p and 2 p + 1 as the mates of pair p.  The lines of mate 1, then those of mate 2; of a mate its chosen hit first --
// without 256 / 2048, with the pair's MAPQ, signed TLEN (positive for the mate that lies first; for mate 1 where both start at
// the same base), YS:i: (the mate's score) and, in a proper pair, YT:Z:CP --, then its other hits in hit order with their own
// flags and MAPQ (a hit number 0 that was not chosen: 256 and MAPQ 0) and TLEN 0.  Every line carries 1, 64 / 128, 8 / 32 for
// the mate, and RNEXT / PNEXT of the mate's chosen hit, or its own where the mate has none; a mate that did not map lies where
// its partner does (SAM's convention).  A line whose alignment came from a rescue window carries YR:i:1.
inline void sam_pair_lines(std::string &out, const State &m, uint64_t p, const kiss_hip_pair &pr)
{
    const uint64_t R = m.ref.names.size();
    const uint32_t chosen[2] = {pr.hit1, pr.hit2}, mapq[2] = {pr.mapq1, pr.mapq2};
    const bool proper = (pr.flags & KISS_HIP_PAIR_PROPER) != 0, mapped[2] = {pr.hit1 != KISS_HIP_PAIR_NONE, pr.hit2 != KISS_HIP_PAIR_NONE};
    bool rev[2] = {false, false}; // where a mate lies: its chosen hit
    std::string rname[2] = {"*", "*"};
    uint64_t pos[2] = {0, 0}, tbeg[2] = {0, 0};
    for (int i = 0; i < 2; i++) {
        if (!mapped[i]) continue;
        const kiss_hip_hit &t = m.hits[chosen[i]];
        rev[i] = (t.flags & KISS_HIP_HIT_REVERSE) != 0;
        if (R) rname[i] = m.ref.names[t.ref];
        tbeg[i] = m.al.alns[t.aln].tbeg;
        pos[i] = tbeg[i] - (R ? m.ref.bounds[t.ref] : 0) + 1;
    }
    for (int i = 0; i < 2; i++) {
        const int o = 1 - i, at = mapped[o] ? o : i; // (at: the mate's place, or this read's own when the mate has none)
        const uint64_t q = 2 * p + (uint64_t)i;
        MateFields f;
        f.flag = 1u | (i ? 128u : 64u) | (mapped[o] ? 0u : 8u) | (mapped[o] && rev[o] ? 32u : 0u);
        if (mapped[at]) f.rnext = &rname[at], f.pnext = pos[at];
        if (!mapped[i]) {
            sam_line(out, m, q, nullptr, f);
            continue;
        }
        const auto line = [&](uint64_t h) {
            MateFields g = f;
            g.rescued = !m.source.empty() && m.source[m.hits[h].aln] >= m.first_alns;
            if (h == chosen[i]) {
                g.chosen = true;
                g.flag |= proper ? 2u : 0u;
                g.mapq = mapq[i];
                if (mapped[o] && pr.tlen) g.tlen = (tbeg[i] < tbeg[o] || (tbeg[i] == tbeg[o] && i == 0)) ? (long long)pr.tlen : -(long long)pr.tlen;
                if (mapped[o]) g.mate_score = m.hits[chosen[o]].score;
                g.proper = proper;
            } else if (h == m.hidx[q]) { // the primary of the read on its own, displaced by the pair
                g.flag |= 256u;
                g.mapq = 0;
            }
            sam_line(out, m, q, &m.hits[h], g);
        };
        line(chosen[i]); // the chosen hit, then the others in hit order
        for (uint64_t h = m.hidx[q]; h < m.hidx[q + 1]; h++)
            if (h != chosen[i]) line(h);
    }
}

// the header: one @SQ per record of the reference
inline void sam_header(std::string &out, const RefRecords &ref, const char *version)
{
    out += "@HD\tVN:1.6\tSO:unsorted\n";
    for (size_t r = 0; r < ref.names.size(); r++)
        out += "@SQ\tSN:" + ref.names[r] + "\tLN:" + std::to_string(ref.bounds[r + 1] - ref.bounds[r]) + '\n';
    out += std::string("@PG\tID:kiss\tPN:kiss\tVN:") + version + '\n';
}

// the lines of every read of the State, or when `paired` of every pair
inline void sam_lines(StdoutWriter &w, const State &s, bool paired)
{
    for (uint64_t i = 0; i < (paired ? s.Q / 2 : s.Q); i++) {
        if (paired && (s.pairs[i].flags & KISS_HIP_PAIR_BAD_INPUT)) // (found here, behind the lines of the pairs before it)
            throw std::runtime_error("kiss_hip_fmi_pair_host: pair " + std::to_string(s.first / 2 + i) + " is bad input");
        if (paired) sam_pair_lines(w.out, s, i, s.pairs[i]);
        else sam_read_lines(w.out, s, i);
        w.flush_if_full();
    }
}

inline void sam_info(const State &s, bool paired, bool rescued);

// SAM: the header, then the lines, then the [info] lines; rescued: --rescue has run
inline int print_sam(const State &s, bool paired, bool rescued, const char *version)
{
    StdoutWriter w;
    sam_header(w.out, s.ref, version);
    sam_lines(w, s, paired);
    w.finish();
    sam_info(s, paired, rescued);
    return 0;
}

// what the select, pair and rescue calls counted
inline void sam_info(const State &s, bool paired, bool rescued)
{
    const kiss_hip_select_report &r = s.select_rep;
    std::fprintf(stderr, "[info] reads: %llu, alignments: %llu, candidates: %llu, spanning: %llu, redundant: %llu, hits: %llu, heads: %llu, mapped: %llu, "
                         "most candidates of a read: %u\n",
                 (ull)s.Q, (ull)r.alignments, (ull)r.candidates, (ull)r.spanning, (ull)r.redundant, (ull)r.hits, (ull)r.heads, (ull)r.mapped, r.max_candidates);
    const kiss_hip_pair_report &pr = s.pair_rep;
    if (paired)
        std::fprintf(stderr, "[info] pairs: %llu, eligible hits: %llu, combinations: %llu, concordant: %llu, proper: %llu, promoted: %llu, lifted: %llu, "
                             "most combinations of a pair: %llu\n",
                     (ull)pr.P, (ull)pr.eligible, (ull)pr.combinations, (ull)pr.concordant, (ull)pr.proper, (ull)pr.promoted, (ull)pr.lifted,
                     (ull)pr.max_combinations);
    uint64_t now_proper = 0; // rescued: the pairs that are proper now and were not before
    for (uint64_t p = 0; rescued && p < s.Q / 2; p++)
        now_proper += (s.pairs[p].flags & KISS_HIP_PAIR_PROPER) && !(s.first_pairs[p].flags & KISS_HIP_PAIR_PROPER) ? 1u : 0u;
    if (rescued)
        std::fprintf(stderr, "[info] rescue: pairs planned: %llu, anchors: %llu, chains: %llu, split: %llu, empty: %llu, bad input: %llu, "
                             "most chains of a pair: %llu, rescued: %llu\n",
                     (ull)s.plan.pairs_planned, (ull)s.plan.anchors, (ull)s.plan.chains, (ull)s.plan.split, (ull)s.plan.empty, (ull)s.plan.bad_input,
                     (ull)s.plan.max_chains, (ull)now_proper);
}

} // namespace kiss_cli
