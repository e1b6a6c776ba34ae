// The printers of `kiss fmindex_query --seeds ...` on a State made by hand (tests/test_cli_format.py has the lines expected):
// kiss_amd/csrc/host/cli_format.hpp alone, no libkiss_hip.
#include "kiss_amd/csrc/host/cli_format.hpp"

using namespace kiss_cli;

static void add_read(State &s, const std::string &name, const std::string &letters)
{
    for (char c : letters) s.rd.reads.push_back(c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4);
    s.rd.ridx.push_back(s.rd.reads.size());
    s.rd.names.push_back(name);
    s.Q++;
}
static uint32_t op(uint32_t n, char what) { return n << 4 | (what == 'M' ? 0u : what == 'I' ? 1u : 2u); }

int main()
{
    // ---- reads on their own, both strands: two records of 100 and 150 bases
    State s;
    s.ref.names = {"chrA", "chrB"};
    s.ref.bounds = {0, 100, 250};
    add_read(s, "r0", "ACGTACGTACGT");
    add_read(s, "r1", "ACGTNACGTACGTAC");
    add_read(s, "r2", "AACCGGTTAC");
    add_read(s, "3", "ACGTACGTAN");
    s.V = 8;
    s.seeds = {{2, 20, 5, 8}, {1, 19, 0, 600}}; // start len sa_beg sa_end: of r0 +, with positions; of r1 -, without
    s.sidx = {0, 1, 1, 1, 2, 2, 2, 2, 2};
    s.pidx = {0, 3, 3};
    s.pos = {7, 9, 11};
    s.seed_rep.seeds = 2, s.seed_rep.located_seeds = 1, s.seed_rep.positions = 3;
    print_seeds(s, true);
    s.ch.chains = {{50, 2, 0, 60, 100, 161}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
    s.ch.cidx = {0, 1, 1, 1, 2, 5, 6, 6, 6}; // r0 +, r1 -, three of r2 +, one of r2 -
    s.chain_rep.anchors = 9, s.chain_rep.chains = 6, s.chain_rep.best_score = 50;
    print_chains(s, true);
    //            score flags rbeg rend tbeg tend matches mismatches ins del gaps band
    s.al.alns = {{12, 0, 0, 12, 10, 22, 12, 0, 0, 0, 0, 0},   // all of r0
                 {6, 0, 2, 12, 120, 129, 8, 1, 1, 0, 1, 0},   // clips on both sides
                 {7, 0, 3, 10, 40, 47, 7, 0, 0, 0, 0, 0},     // a clip on the left
                 {6, 0, 0, 6, 140, 146, 6, 0, 0, 0, 0, 0},    // a clip on the right
                 {5, 0, 0, 7, 200, 208, 7, 0, 0, 1, 1, 0},
                 {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};       // nothing aligned
    s.al.cigar = {op(12, 'M'), op(5, 'M'), op(1, 'I'), op(4, 'M'), op(7, 'M'), op(6, 'M'), op(4, 'M'), op(1, 'D'), op(3, 'M')};
    s.al.oidx = {0, 1, 4, 5, 6, 9, 9};
    s.al.rep.chains = 6, s.al.rep.aligned = 5, s.al.rep.too_wide = 1, s.al.rep.best_score = 12;
    print_alignments(s, true);
    //          aln flags mapq score sub n_sec head ref
    s.hits = {{0, 0, 60, 12, 0, 0, 0, 0},
              {1, KISS_HIP_HIT_REVERSE, 37, 6, 3, 0, 1, 1},
              {2, 0, 20, 7, 6, 1, 2, 0},
              {3, KISS_HIP_HIT_SECONDARY, 0, 6, 0, 0, 2, 1},
              {4, KISS_HIP_HIT_SUPPLEMENTARY | KISS_HIP_HIT_REVERSE, 11, 5, 2, 0, 4, 1}};
    s.hidx = {0, 1, 2, 5, 5};
    s.select_rep.alignments = 6, s.select_rep.candidates = 5, s.select_rep.hits = 5, s.select_rep.heads = 4, s.select_rep.mapped = 3;
    s.select_rep.max_candidates = 3;
    print_sam(s, false, false, "X");
    s.ref = RefRecords(); // no records: RNAME is *, POS counts from the start of the text
    print_sam(s, false, false, "X");
    // ---- pairs: six of them, every read ACGTACGTAC and aligned as 10M
    State p;
    p.ref.names = {"chrA", "chrB"};
    p.ref.bounds = {0, 100, 250};
    for (int q = 0; q < 12; q++) add_read(p, "p" + std::to_string(q / 2), "ACGTACGTAC");
    for (uint32_t tbeg : {10, 50, 30, 30, 5, 200, 110, 60, 160, 190}) {
        p.al.oidx.push_back(p.al.alns.size());
        p.al.alns.push_back({10, 0, 0, 10, tbeg, tbeg + 10, 10, 0, 0, 0, 0, 0});
        p.al.cigar.push_back(op(10, 'M'));
    }
    p.al.oidx.push_back(p.al.alns.size());
    p.hits = {{0, 0, 60, 10, 0, 0, 0, 0},   {1, KISS_HIP_HIT_REVERSE, 60, 10, 0, 0, 1, 0},  // a proper pair
              {2, 0, 30, 10, 1, 0, 2, 0},   {3, KISS_HIP_HIT_REVERSE, 31, 10, 2, 0, 3, 0},  // both start at the same base
              {4, 0, 60, 10, 0, 0, 4, 0},   {5, 0, 59, 10, 0, 0, 5, 1},                     // on two records
              {6, KISS_HIP_HIT_REVERSE, 50, 9, 4, 0, 6, 1},                                 // the mate does not map
              {7, 0, 3, 10, 10, 1, 7, 0},   {8, KISS_HIP_HIT_SECONDARY, 0, 10, 0, 0, 7, 1}, // the pair chose the secondary
              {9, KISS_HIP_HIT_REVERSE, 22, 8, 0, 0, 9, 1}};                                // (its mate, from a rescue window)
    p.hidx = {0, 1, 2, 3, 4, 5, 6, 7, 7, 7, 7, 9, 10};
    p.source = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};
    p.first_alns = 9;
    const uint32_t none = KISS_HIP_PAIR_NONE;
    //         hit1 hit2 flags tlen score sub1 sub2 mapq1 mapq2 n_conc
    p.pairs = {{0, 1, KISS_HIP_PAIR_PROPER, 50, 20, 0, 0, 40, 41, 1}, {2, 3, 0, 10, 20, 0, 0, 12, 13, 0},
               {4, 5, 0, 0, 20, 0, 0, 60, 59, 0},                     {6, none, 0, 0, 9, 0, 0, 50, 0, 0},
               {none, none, 0, 0, 0, 0, 0, 0, 0, 0},                  {8, 9, KISS_HIP_PAIR_PROPER, 40, 18, 0, 0, 25, 26, 1}};
    p.first_pairs = p.pairs;
    p.first_pairs[5].flags = 0; // (the last pair was not proper before the rescue)
    p.select_rep.alignments = 10, p.select_rep.hits = 10;
    p.pair_rep.P = 6, p.pair_rep.proper = 2, p.pair_rep.promoted = 1;
    p.plan.pairs_planned = 4, p.plan.anchors = 3, p.plan.chains = 1, p.plan.max_chains = 1;
    return print_sam(p, true, true, "X");
}
