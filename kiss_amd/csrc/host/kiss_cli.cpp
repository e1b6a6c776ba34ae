// kiss_cli.cpp -- `kiss`: the kISS command line on top of libkiss_hip.so (host C++17, no HIP, no Boost).
//
// Keeps the reference's CLI surface (reference include/utils/options.hpp:83-203, src/main.cpp:19-39):
//   kiss [-h] [-v] [-g] [-t NUM] [--verbose] <command> [options] <FASTA filename/Text filename>
//   suffix_sort    [-k NUM(=256, -1 = unbounded)] [-s PARALLEL_SORTING|PREFIX_DOUBLING]   (command/suffix_sort.hpp)
//   fmindex_build  [-k NUM (ignored, like the reference)]  -> writes <fasta>.fmi            (command/fmindex_build.hpp)
//   fmindex_query  [-q STR] [-n NUM(=10)] [-b patterns.bin]                                  (command/fmindex_query.hpp)
//   (opt-in: fmindex_build --sa-intv N --lookup-len L, fmindex_query --sa-intv N: FMIndex<N>{.LOOKUP_LEN = L}; the
//    defaults 4 and 0 are the reference CLI's; the query reads L from the file, which does not record N)
//   (opt-in: fmindex_query --mismatches E, E in 0..3: every position within Hamming distance E of the query, ascending,
//    each with its mismatch count (kiss_hip_fmi_query_mm_host); the positions need an index of the EXACT suffix array:
//    fmindex_build --exact, same .fmi layout)
//   (opt-in: fmindex_query --seeds READS [--min-seed-len N] [--max-seed-len M] [--max-occ N] [--both-strands]: the maximal
//    exact match seeds of every read of READS (one read per line, ACGTacgt, any other letter is no base; lines starting
//    with '>' and empty lines are skipped), one line per seed on stdout: read strand start len count pos...; also needs
//    fmindex_build --exact; with --chain [--max-gap N] [--band N] [--gap-cost N] [--max-lookback N] [--min-chain-score N] the
//    positions of the seeds of a read are chained into candidate loci (kiss_hip_fmi_chain_host) and the output is one line
//    per chain instead: read strand score anchors rbeg rend tbeg tend; with --align on top [--match N] [--mismatch N]
//    [--gap-open N] [--gap-extend N] [--align-band N] every chain is aligned to the text (kiss_hip_fmi_align_host: banded,
//    and with --sam on top [--min-map-score N] [--overlap N] [--mapq-coef N] [--mapq-max N] [--max-hits N] the alignments of
//    a read are turned into its mappings (kiss_hip_fmi_select_host) and stdout is SAM: one line per hit, one per unmapped read;
//    with --mates READS2 on top [--ins-min N] [--ins-max N] [--ins-mean N] [--pair-pen-coef N] [--pair-pen-max N] read p of
//    READS and read p of READS2 are the two mates of pair p (forward-then-reverse libraries; both strands are searched): their
//    mappings are paired (kiss_hip_fmi_pair_host) and the SAM is paired -- the lines of the two mates adjacent, the chosen hit
//    of a mate first with the pair's MAPQ, flags 1 / 2 / 8 / 32 / 64 / 128, RNEXT, PNEXT, signed TLEN, YS:i: and YT:Z:CP;
//    with --rescue on top [--rescue-anchors N] [--rescue-min-anchor-score N] [--rescue-width N] the mates of a pair that is not
//    proper are aligned once more inside the windows next to their partner's hits (kiss_hip_fmi_rescue_host, the align call,
//    kiss_hip_fmi_aln_merge_host), select and pair run again, and a line that came from a window carries YR:i:1;
//    affine gaps, local) and the line of a chain is: read strand score rbeg rend tbeg tend nm cigar)
//   (-g / --generic: the file is a text over the byte alphabet, taken byte for byte -- no FASTA rule, no newline stripping,
//    no % 4.  suffix_sort gives the exact suffix array (kiss_hip_suffix_sort_u8; -k and -s are ignored) and, with
//    --output-lcp, its LCP array; fmindex_build writes <file>.fmi8 (kiss_hip_fmi8_build_host);
//    fmindex_query reads it: -q STR is the bytes of STR, -b patterns.bin holds raw bytes.  One device, no lookup table, no
//    mismatches.  The reference rejects -g in all three commands: command/*.hpp:15-18.)
// and its log fields ("n = …, k = …, suffix sorting elapsed …", "query = … found N times", "searching time",
// "number of matched locations", "location checksum").  Extras (opt-in): --output-sa FILE (raw u32 LE, n+1
// entries; the reference never writes the SA), --output-lcp FILE (the LCP array of an exact suffix array, same format), --device N, and for suffix_sort --gpus N / --devices LIST (the LMS sort
// sharded over several GPUs of the node by ONE process, kiss_hip_multi_*; include/kiss_hip.h).
// Input handling as utils/io.hpp:6-18 + suffix_sort.hpp:33: FASTA if the first byte is '>' (all records
// concatenated), else plain text lines; ACGT/acgt -> 0..3, every other character -> 4 % 4 = 0 (A).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/kiss_hip.h"

namespace {

const char *VERSION = "1.0.0-hip";

void usage()
{
    std::cerr << "kiss " << VERSION << " (MI355X / libkiss_hip)\n"
              << "kiss [--generic-option ...] cmd [--cmd-specific-option ...]\n"
              << "Generic options:\n"
              << "  -h [ --help ]            produce help message\n"
              << "  -v [ --version ]         print version string\n"
              << "  -g [ --generic ]         the file is a text over the byte alphabet, byte for byte: exact suffix array\n"
              << "                           (-k, -s ignored), FILE.fmi8 index; not with --gpus, --lookup-len, --exact, --mismatches\n"
              << "  -t [ --num_threads ] NUM accepted for compatibility; no result depends on it\n"
              << "  --verbose                print per-stage device times\n"
              << "  --device NUM             HIP device index (default 0)\n\n"
              << "./kiss suffix_sort [--option ...] <FASTA filename/Text filename>\n"
              << "  -k [ --kordered ] NUM (=256)   k-ordered value; -1 indicates unbounded sorting\n"
              << "  -s [ --sorting-algorithm ] ALGO (=PARALLEL_SORTING)   PARALLEL_SORTING or PREFIX_DOUBLING\n"
              << "  --output-sa FILE               also write the suffix array (raw uint32 LE, n+1 entries)\n"
              << "  --output-lcp FILE              also write the LCP array (raw uint32 LE, n+1 entries); exact order only (-k -1)\n"
              << "  --gpus NUM (=1)                shard the LMS sort over NUM devices (--device, --device + 1, ...)\n"
              << "  --devices LIST                 the same with an explicit comma-separated device list\n\n"
              << "./kiss fmindex_build [--option ...] <FASTA filename/Text filename>\n"
              << "  -k [ --kordered ] NUM (=256)   accepted and ignored (the index is built with k = 32)\n"
              << "  --sa-intv NUM (=4)             SA sampling interval, 1..32 (1: the whole SA)\n"
              << "  --lookup-len NUM (=0)          k-mer lookup table of 4^NUM ranges, 0..14\n"
              << "  --exact                        build from the exact suffix array (k = -1) instead of k = 32: what the\n"
              << "                                 positions of fmindex_query --mismatches need; same .fmi layout\n\n"
              << "./kiss fmindex_query [--option ...] <FASTA filename/Text filename>\n"
              << "  -q [ --query ] STR             content of the query string\n"
              << "  -n [ --headn ] NUM (=10)       output the first n locations in single query mode\n"
              << "  -b [ --batch ] patterns.bin    batch query mode (u32 len, u32 count, then count x len bytes)\n"
              << "  --sa-intv NUM (=4)             the SA sampling interval the index was built with\n"
              << "  --mismatches NUM               also report the locations with up to NUM (0..3) substitutions; the\n"
              << "                                 positions need an index built with fmindex_build --exact\n"
              << "  --seeds READS                  the maximal exact match seeds of the reads of READS (one per line, ACGT,\n"
              << "                                 any other letter is no base; '>' lines are skipped) on stdout, one line\n"
              << "                                 per seed: read strand(+/-) start len count pos...; the positions need an\n"
              << "                                 index built with fmindex_build --exact; not with -g, -q, -b, --mismatches\n"
              << "  --min-seed-len NUM (=19)       shortest seed reported\n"
              << "  --max-seed-len NUM (=0)        longest match followed (0: no cap)\n"
              << "  --max-occ NUM (=500)           seeds with more occurrences get no positions (0: no limit)\n"
              << "  --both-strands                 also the reverse complement of every read (strand -)\n"
              << "  --chain                        with --seeds: chain the seed positions of every read into candidate loci\n"
              << "                                 and print one line per chain instead: read strand score anchors rbeg rend\n"
              << "                                 tbeg tend\n"
              << "  --max-gap NUM (=5000)          largest step between two anchors of a chain, in the read and in the text\n"
              << "  --band NUM (=500)              largest difference between the two steps\n"
              << "  --gap-cost NUM (=2)            eighths of a point taken off per base of that difference\n"
              << "  --max-lookback NUM (=64)       predecessors tried per anchor (0: no bound)\n"
              << "  --min-chain-score NUM (=40)    lowest score of a chain reported\n"
              << "  --align                        with --chain: align every chain to the text (banded, affine gaps, local) and\n"
              << "                                 print per chain: read strand score rbeg rend tbeg tend nm cigar (SAM style\n"
              << "                                 with S clips; * when nothing aligns)\n"
              << "  --match NUM (=1)               score of a matching column\n"
              << "  --mismatch NUM (=4)            penalty of a mismatching column\n"
              << "  --gap-open NUM (=6)            a gap of g bases costs gap-open + g * gap-extend\n"
              << "  --gap-extend NUM (=1)\n"
              << "  --align-band NUM (=32)         diagonals aligned on either side of the chain's own\n"
              << "  --sam                          with --align: pick the mappings of every read (primary, secondary,\n"
              << "                                 supplementary, MAPQ) and print SAM instead: a header with one @SQ per record\n"
              << "                                 of the reference file, one line per hit, one line (FLAG 4) per unmapped read\n"
              << "  --min-map-score NUM (=30)      lowest alignment score of a mapping\n"
              << "  --overlap NUM (=128)           share of the shorter interval, in 256ths (0..256), above which two\n"
              << "                                 alignments are the same locus (in the text) or compete (in the read)\n"
              << "  --mapq-coef NUM (=120)         MAPQ = min(mapq-max, mapq-coef * (score - best secondary) / score)\n"
              << "  --mapq-max NUM (=60)\n"
              << "  --max-hits NUM (=0)            hits written per read (0: all)\n"
              << "  --mates READS2                 with --sam: read p of READS2 is the mate of read p of READS (forward-then-\n"
              << "                                 reverse libraries; implies --both-strands); the mappings of the two are paired\n"
              << "                                 and the SAM is paired: the mates adjacent, the chosen hit of a mate first, with\n"
              << "                                 the pair's MAPQ, the mate fields, signed TLEN, YS:i: and, in a proper pair, YT:Z:CP\n"
              << "  --ins-min NUM (=0)             shortest insert (first base of the forward mate to the last of the reverse one)\n"
              << "  --ins-max NUM (=1000)          longest insert of a proper pair\n"
              << "  --ins-mean NUM (=400)          the insert that costs nothing\n"
              << "  --pair-pen-coef NUM (=8)       256ths of a score point taken off per base of deviation from --ins-mean\n"
              << "  --pair-pen-max NUM (=20)       most points taken off\n"
              << "  --rescue                       with --mates: a mate of a pair that is not proper is aligned once more, inside the\n"
              << "                                 window that --ins-min / --ins-max leave next to the hits of its partner; the\n"
              << "                                 mappings are picked and paired again with what that finds (lines from it: YR:i:1)\n"
              << "  --rescue-anchors NUM (=4)      hits of the partner a window is laid next to\n"
              << "  --rescue-min-anchor-score NUM (=0)  lowest score of such a hit\n"
              << "  --rescue-width NUM (=960)      diagonals of a window aligned in one piece (1..1024)\n";
}

inline uint8_t to_code(unsigned char c)
{
    switch (c) {
    case 'a': case 'A': return 0;
    case 'c': case 'C': return 1;
    case 'g': case 'G': return 2;
    case 't': case 'T': return 3;
    default: return 0; // Codec::to_int gives 4, the commands apply % 4 (suffix_sort.hpp:33)
    }
}

void check(int rc, const char *where)
{
    if (rc != KISS_HIP_OK) throw std::runtime_error(std::string(where) + ": " + kiss_hip_strerror(rc));
}

// utils/io.hpp:6-18 (read_sequence) + the `% 4` of the commands: the file is streamed to the device and parsed there
// (kiss_amd/csrc/fasta.hip); the host never touches a base
struct DeviceText {
    kiss_hip_ctx *ctx = nullptr;
    uint8_t *d_S = nullptr;
    uint64_t n = 0;
    double create_s = 0, load_s = 0;
    bool own_ctx = true;
    // borrowed != nullptr: load through a context that something else owns (the first device's context of a
    // kiss_hip_multi: one set of work arrays serves the loader and the sort; allocating a second set after freeing the
    // first costs seconds on this driver -- profiles/r03_first_call_allocation_times_*.log)
    DeviceText(const std::string &path, int device, kiss_hip_ctx *borrowed = nullptr)
    {
        uint64_t bytes = 0;
        if (kiss_hip_file_size(path.c_str(), &bytes) != KISS_HIP_OK) throw std::runtime_error("cannot open " + path);
        auto t0 = std::chrono::steady_clock::now();
        if (borrowed) {
            ctx = borrowed;
            own_ctx = false;
        } else {
            check(kiss_hip_ctx_create(&ctx, device, bytes ? bytes : 1), "kiss_hip_ctx_create");
        }
        create_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        t0 = std::chrono::steady_clock::now();
        const int rc = kiss_hip_ctx_load_text_file(ctx, path.c_str(), &d_S, &n);
        load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (rc != KISS_HIP_OK) {
            if (own_ctx) kiss_hip_ctx_destroy(ctx);
            throw std::runtime_error(std::string("kiss_hip_ctx_load_text_file: ") + kiss_hip_strerror(rc));
        }
    }
    std::vector<uint8_t> to_host() const
    {
        std::vector<uint8_t> S(n);
        check(kiss_hip_copy_to_host(S.data(), d_S, n), "kiss_hip_copy_to_host");
        return S;
    }
    ~DeviceText()
    {
        kiss_hip_free_dev(d_S);
        if (ctx && own_ctx) kiss_hip_ctx_destroy(ctx);
    }
    DeviceText(const DeviceText &) = delete;
    DeviceText &operator=(const DeviceText &) = delete;
};

struct Args {
    std::string command, fasta, query, batch, output_sa, output_lcp, algo = "PARALLEL_SORTING";
    long long k = 256;
    size_t headn = 10;
    uint32_t sa_intv = 4, lookup_len = 0; // FMIndex<SA_INTV>{.LOOKUP_LEN}: the reference CLI's (fmindex_build.hpp:27-29)
    int device = 0, gpus = 1;
    std::vector<int> devices; // --devices; empty: device, device + 1, ... (gpus of them)
    bool verbose = false, generic = false, exact = false;
    std::vector<std::string> seen; // the long names of the options given (what -g refuses is named)
    int mismatches = -1; // fmindex_query --mismatches (-1: the exact query of the reference)
    std::string seeds;   // fmindex_query --seeds READS
    uint32_t min_seed_len = 19, max_seed_len = 0, max_occ = 500;
    bool both_strands = false;
    bool chain = false; // fmindex_query --seeds READS --chain
    kiss_hip_chain_params chain_params{5000, 500, 2, 64, 40};
    bool align = false; // fmindex_query --seeds READS --chain --align
    kiss_hip_align_params align_params{1, 4, 6, 1, 32};
    bool sam = false; // fmindex_query --seeds READS --chain --align --sam
    kiss_hip_select_params select_params{30, 128, 120, 60, 0};
    std::string mates; // fmindex_query --seeds READS --mates READS2 --chain --align --sam
    kiss_hip_pair_params pair_params{0, 1000, 400, 8, 20, 120, 60};
    bool rescue = false; // fmindex_query ... --mates READS2 --sam --rescue
    kiss_hip_rescue_params rescue_params{0, 1000, 4, 0, 960}; // (ins_min / ins_max: the pair parameters')
};

Args parse(int argc, char **argv)
{
    Args a;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        std::string s = argv[i];
        auto next = [&](const char *name) -> std::string {
            if (i + 1 >= argc) throw std::runtime_error(std::string("the required argument for option '") + name + "' is missing");
            return argv[++i];
        };
        if (s == "--gpus" || s == "--devices" || s == "--lookup-len" || s == "--exact" || s == "--mismatches" || s == "--sa-intv" ||
            s == "--seeds" || s == "--min-seed-len" || s == "--max-seed-len" || s == "--max-occ" || s == "--both-strands" || s == "--chain" ||
            s == "--max-gap" || s == "--band" || s == "--gap-cost" || s == "--max-lookback" || s == "--min-chain-score" ||
            s == "--align" || s == "--match" || s == "--mismatch" || s == "--gap-open" || s == "--gap-extend" || s == "--align-band" ||
            s == "--sam" || s == "--min-map-score" || s == "--overlap" || s == "--mapq-coef" || s == "--mapq-max" || s == "--max-hits" ||
            s == "--mates" || s == "--ins-min" || s == "--ins-max" || s == "--ins-mean" || s == "--pair-pen-coef" || s == "--pair-pen-max" ||
            s == "--rescue" || s == "--rescue-anchors" || s == "--rescue-min-anchor-score" || s == "--rescue-width")
            a.seen.push_back(s);
        if (s == "-k" || s == "--kordered") a.seen.push_back("--kordered");
        if (s == "-s" || s == "--sorting-algorithm") a.seen.push_back("--sorting-algorithm");
        if (s == "-h" || s == "--help") { usage(); std::exit(1); }
        else if (s == "-v" || s == "--version") { std::cerr << VERSION << std::endl; std::exit(1); }
        else if (s == "-g" || s == "--generic") a.generic = true;
        else if (s == "--verbose") a.verbose = true;
        else if (s == "-t" || s == "--num_threads") (void)next("--num_threads");
        else if (s == "--device") a.device = std::stoi(next("--device"));
        else if (s == "-k" || s == "--kordered") a.k = std::stoll(next("--kordered"));
        else if (s == "-s" || s == "--sorting-algorithm") a.algo = next("--sorting-algorithm");
        else if (s == "-q" || s == "--query") a.query = next("--query");
        else if (s == "-n" || s == "--headn") a.headn = (size_t)std::stoull(next("--headn"));
        else if (s == "-b" || s == "--batch") a.batch = next("--batch");
        else if (s == "--output-sa") a.output_sa = next("--output-sa");
        else if (s == "--output-lcp") a.output_lcp = next("--output-lcp");
        else if (s == "--sa-intv") a.sa_intv = (uint32_t)std::stoul(next("--sa-intv"));
        else if (s == "--lookup-len") a.lookup_len = (uint32_t)std::stoul(next("--lookup-len"));
        else if (s == "--gpus") a.gpus = std::stoi(next("--gpus"));
        else if (s == "--exact") a.exact = true;
        else if (s == "--mismatches") a.mismatches = std::stoi(next("--mismatches"));
        else if (s == "--seeds") a.seeds = next("--seeds");
        else if (s == "--min-seed-len") a.min_seed_len = (uint32_t)std::stoul(next("--min-seed-len"));
        else if (s == "--max-seed-len") a.max_seed_len = (uint32_t)std::stoul(next("--max-seed-len"));
        else if (s == "--max-occ") a.max_occ = (uint32_t)std::stoul(next("--max-occ"));
        else if (s == "--both-strands") a.both_strands = true;
        else if (s == "--chain") a.chain = true;
        else if (s == "--max-gap") a.chain_params.max_gap = (uint32_t)std::stoul(next("--max-gap"));
        else if (s == "--band") a.chain_params.band = (uint32_t)std::stoul(next("--band"));
        else if (s == "--gap-cost") a.chain_params.gap_cost = (uint32_t)std::stoul(next("--gap-cost"));
        else if (s == "--max-lookback") a.chain_params.max_lookback = (uint32_t)std::stoul(next("--max-lookback"));
        else if (s == "--min-chain-score") a.chain_params.min_score = (uint32_t)std::stoul(next("--min-chain-score"));
        else if (s == "--align") a.align = true;
        else if (s == "--match") a.align_params.match = (uint32_t)std::stoul(next("--match"));
        else if (s == "--mismatch") a.align_params.mismatch = (uint32_t)std::stoul(next("--mismatch"));
        else if (s == "--gap-open") a.align_params.gap_open = (uint32_t)std::stoul(next("--gap-open"));
        else if (s == "--gap-extend") a.align_params.gap_extend = (uint32_t)std::stoul(next("--gap-extend"));
        else if (s == "--align-band") a.align_params.band = (uint32_t)std::stoul(next("--align-band"));
        else if (s == "--sam") a.sam = true;
        else if (s == "--min-map-score") a.select_params.min_score = (uint32_t)std::stoul(next("--min-map-score"));
        else if (s == "--overlap") a.select_params.overlap = (uint32_t)std::stoul(next("--overlap"));
        else if (s == "--mapq-coef") a.select_params.mapq_coef = (uint32_t)std::stoul(next("--mapq-coef"));
        else if (s == "--mapq-max") a.select_params.mapq_max = (uint32_t)std::stoul(next("--mapq-max"));
        else if (s == "--max-hits") a.select_params.max_hits = (uint32_t)std::stoul(next("--max-hits"));
        else if (s == "--mates") a.mates = next("--mates");
        else if (s == "--ins-min") a.pair_params.ins_min = (uint32_t)std::stoul(next("--ins-min"));
        else if (s == "--ins-max") a.pair_params.ins_max = (uint32_t)std::stoul(next("--ins-max"));
        else if (s == "--ins-mean") a.pair_params.ins_mean = (uint32_t)std::stoul(next("--ins-mean"));
        else if (s == "--pair-pen-coef") a.pair_params.pen_coef = (uint32_t)std::stoul(next("--pair-pen-coef"));
        else if (s == "--pair-pen-max") a.pair_params.pen_max = (uint32_t)std::stoul(next("--pair-pen-max"));
        else if (s == "--rescue") a.rescue = true;
        else if (s == "--rescue-anchors") a.rescue_params.max_anchors = (uint32_t)std::stoul(next("--rescue-anchors"));
        else if (s == "--rescue-min-anchor-score") a.rescue_params.min_anchor_score = (uint32_t)std::stoul(next("--rescue-min-anchor-score"));
        else if (s == "--rescue-width") a.rescue_params.max_width = (uint32_t)std::stoul(next("--rescue-width"));
        else if (s == "--devices") {
            const std::string list = next("--devices");
            size_t at = 0;
            while (at <= list.size()) {
                const size_t comma = list.find(',', at);
                const std::string item = list.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
                if (item.empty()) throw std::runtime_error("--devices: empty entry in '" + list + "'");
                a.devices.push_back(std::stoi(item));
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
        }
        else if (!s.empty() && s[0] == '-' && s.size() > 1) throw std::runtime_error("unrecognised option '" + s + "'");
        else pos.push_back(s);
    }
    if (pos.empty()) { usage(); std::exit(1); }
    if (a.gpus < 1) throw std::runtime_error("--gpus must be >= 1");
    if (a.sa_intv < 1 || a.sa_intv > KISS_HIP_FMI_MAX_SA_INTV) throw std::runtime_error("--sa-intv must be in 1..32");
    if (a.lookup_len > KISS_HIP_FMI_MAX_LOOKUP_LEN) throw std::runtime_error("--lookup-len must be in 0..14");
    if (a.mismatches < -1 || a.mismatches > (int)KISS_HIP_FMI_MAX_MISMATCHES) throw std::runtime_error("--mismatches must be in 0..3");
    {
        const auto given_here = [&](const char *o) { return std::find(a.seen.begin(), a.seen.end(), o) != a.seen.end(); };
        for (const char *o : {"--min-seed-len", "--max-seed-len", "--max-occ", "--both-strands"})
            if (given_here(o) && !given_here("--seeds")) throw std::runtime_error(std::string(o) + " goes with --seeds");
        for (const char *o : {"--max-gap", "--band", "--gap-cost", "--max-lookback", "--min-chain-score"})
            if (given_here(o) && !given_here("--chain")) throw std::runtime_error(std::string(o) + " goes with --chain");
        for (const char *o : {"--align", "--match", "--mismatch", "--gap-open", "--gap-extend", "--align-band"})
            if (given_here(o) && !given_here("--chain")) throw std::runtime_error(std::string(o) + " goes with --chain");
        for (const char *o : {"--match", "--mismatch", "--gap-open", "--gap-extend", "--align-band"})
            if (given_here(o) && !given_here("--align")) throw std::runtime_error(std::string(o) + " goes with --align");
        if (given_here("--chain") && !given_here("--seeds")) throw std::runtime_error("--chain goes with --seeds");
        if (given_here("--sam") && !given_here("--align")) throw std::runtime_error("--sam goes with --align");
        for (const char *o : {"--min-map-score", "--overlap", "--mapq-coef", "--mapq-max", "--max-hits"})
            if (given_here(o) && !given_here("--sam")) throw std::runtime_error(std::string(o) + " goes with --sam");
        if (a.select_params.overlap > 256u || a.select_params.mapq_coef > 65535u || a.select_params.mapq_max > 255u)
            throw std::runtime_error("--overlap is at most 256, --mapq-coef at most 65535, --mapq-max at most 255");
        if (given_here("--mates") && !given_here("--sam")) throw std::runtime_error("--mates goes with --sam");
        for (const char *o : {"--ins-min", "--ins-max", "--ins-mean", "--pair-pen-coef", "--pair-pen-max"})
            if (given_here(o) && !given_here("--mates")) throw std::runtime_error(std::string(o) + " goes with --mates");
        if (a.pair_params.ins_min > a.pair_params.ins_max || a.pair_params.pen_coef > 65535u || a.pair_params.pen_max > 65535u)
            throw std::runtime_error("--ins-min is at most --ins-max, --pair-pen-coef and --pair-pen-max at most 65535");
        if (given_here("--rescue") && !given_here("--mates")) throw std::runtime_error("--rescue goes with --mates");
        for (const char *o : {"--rescue-anchors", "--rescue-min-anchor-score", "--rescue-width"})
            if (given_here(o) && !given_here("--rescue")) throw std::runtime_error(std::string(o) + " goes with --rescue");
        if (a.rescue_params.max_anchors < 1 || a.rescue_params.max_width < 1 || a.rescue_params.max_width > KISS_HIP_ALIGN_MAX_BAND)
            throw std::runtime_error("--rescue-anchors is at least 1, --rescue-width in 1..1024");
        a.rescue_params.ins_min = a.pair_params.ins_min;
        a.rescue_params.ins_max = a.pair_params.ins_max;
        if (given_here("--mates")) { // the pair's MAPQ is on the scale of the reads'; the mates face each other
            a.both_strands = true;
            a.pair_params.mapq_coef = a.select_params.mapq_coef;
            a.pair_params.mapq_max = a.select_params.mapq_max;
        }
        if (a.align_params.match < 1 || a.align_params.match > 65535u || a.align_params.mismatch > 65535u ||
            a.align_params.gap_open > 65535u || a.align_params.gap_extend > 65535u || a.align_params.band > 0x7FFFFFFFu)
            throw std::runtime_error("--match is in 1..65535, --mismatch, --gap-open and --gap-extend are at most 65535, "
                                     "--align-band at most 2147483647");
        if (a.chain_params.max_gap > 0x7FFFFFFFu || a.chain_params.band > 0x7FFFFFFFu || a.chain_params.gap_cost > 65535u)
            throw std::runtime_error("--max-gap and --band are at most 2147483647, --gap-cost at most 65535");
        if (given_here("--seeds")) {
            if (a.generic) throw std::runtime_error("--seeds is not supported for byte texts (--generic)");
            if (!a.query.empty() || !a.batch.empty() || a.mismatches >= 0)
                throw std::runtime_error("--seeds cannot be combined with -q, -b or --mismatches");
            if (a.min_seed_len < 1) throw std::runtime_error("--min-seed-len must be at least 1");
        }
    }
    if (a.devices.empty())
        for (int g = 0; g < a.gpus; g++) a.devices.push_back(a.device + g);
    else
        a.device = a.devices[0]; // the text is loaded, and the induction runs, on the first device of the list
    a.command = pos[0];
    if (!a.seeds.empty() && a.command != "fmindex_query") throw std::runtime_error("--seeds is an option of fmindex_query");
    if (pos.size() < 2) throw std::runtime_error("the option '--fasta' is required but missing");
    a.fasta = pos[1];
    std::transform(a.algo.begin(), a.algo.end(), a.algo.begin(), [](unsigned char c) { return (char)std::toupper(c); });
    return a;
}

double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// `total` u32 of a device buffer into a file (raw little-endian), in pieces
void write_dev_u32(const std::string &path, const void *d_src, uint64_t total)
{
    std::ofstream o(path, std::ios::binary);
    if (!o) throw std::runtime_error("cannot write " + path);
    const uint64_t chunk = 64ull << 20; // entries per piece
    std::vector<uint32_t> buf((size_t)std::min<uint64_t>(total, chunk));
    for (uint64_t off = 0; off < total; off += chunk) {
        const uint64_t c = std::min<uint64_t>(chunk, total - off);
        check(kiss_hip_copy_to_host(buf.data(), (const uint32_t *)d_src + off, c * sizeof(uint32_t)), "kiss_hip_copy_to_host");
        o.write(reinterpret_cast<const char *>(buf.data()), (std::streamsize)(c * sizeof(uint32_t)));
    }
}

// ---- .fmi (fm_index.hpp:591-646; Serializer: u64 count + raw bytes, nothing when the count is 0) ----------
// order: cnt, pri, bwt, occ1, occ2, sa_, lookup_, then b_ and b_occ_ only if SA_INTV != 1
struct Fmi {
    kiss_hip_fmi_sizes_ex zx{};
    const kiss_hip_fmi_sizes &z = zx.base;
    uint32_t sa_intv = 4, lookup_len = 0;
    uint32_t cnt[4]{}, pri = 0;
    std::vector<uint8_t> bwt, occ2;
    std::vector<uint32_t> occ1, sa, b_occ, lookup;
    std::vector<uint64_t> b;
    Fmi(uint32_t sa_intv_, uint32_t lookup_len_) : sa_intv(sa_intv_), lookup_len(lookup_len_) {}
    bool classic() const { return sa_intv == 4 && lookup_len == 0; } // the original entry points
    void alloc(uint64_t n)
    {
        check(kiss_hip_fmi_sizes_ex_for(n, sa_intv, lookup_len, &zx), "kiss_hip_fmi_sizes_ex_for");
        bwt.assign(z.bwt_bytes, 0);
        occ1.assign(z.occ1_entries, 0);
        occ2.assign(z.occ2_bytes, 0);
        sa.assign(z.sa_entries, 0);
        b.assign(z.b_words, 0);
        b_occ.assign(z.b_occ_entries, 0);
        lookup.assign(zx.lookup_entries, 0);
        lookup.back() = (uint32_t)z.n_sa; // LOOKUP_LEN = 0: {0, N} (fm_index.hpp:238-258)
    }
    static void put(std::ofstream &o, uint64_t count, const void *p, uint64_t bytes)
    {
        if (!count) return;
        o.write(reinterpret_cast<const char *>(&count), 8);
        o.write(reinterpret_cast<const char *>(p), (std::streamsize)bytes);
    }
    void save(const std::string &path) const
    {
        std::ofstream o(path, std::ios::binary);
        if (!o) throw std::runtime_error("cannot write " + path);
        o.write(reinterpret_cast<const char *>(cnt), 16);
        o.write(reinterpret_cast<const char *>(&pri), 4);
        put(o, z.n_sa, bwt.data(), z.bwt_bytes);
        put(o, z.occ1_entries / 4, occ1.data(), z.occ1_entries * 4);
        put(o, z.occ2_bytes / 4, occ2.data(), z.occ2_bytes);
        put(o, z.sa_entries, sa.data(), z.sa_entries * 4);
        put(o, lookup.size(), lookup.data(), lookup.size() * 4);
        if (sa_intv != 1) {
            put(o, z.n_sa, b.data(), z.b_words * 8);
            put(o, z.b_occ_entries, b_occ.data(), z.b_occ_entries * 4);
        }
    }
    static uint64_t get_count(std::ifstream &in)
    {
        uint64_t c = 0;
        in.read(reinterpret_cast<char *>(&c), 8);
        if (!in) throw std::runtime_error("truncated .fmi");
        return c;
    }
    // the file does not record SA_INTV (a template parameter of the reference): a file whose counts do not fit the
    // caller's is an error; LOOKUP_LEN follows from the lookup_ count
    void load(const std::string &path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("cannot open " + path + " (run fmindex_build first)");
        in.read(reinterpret_cast<char *>(cnt), 16);
        in.read(reinterpret_cast<char *>(&pri), 4);
        const uint64_t N = get_count(in);
        if (N == 0) throw std::runtime_error("empty .fmi");
        std::vector<uint8_t> bwt_in((N + 3) / 4);
        in.read(reinterpret_cast<char *>(bwt_in.data()), (std::streamsize)bwt_in.size());
        const uint64_t c_occ1 = get_count(in);
        std::vector<uint32_t> occ1_in(c_occ1 * 4);
        in.read(reinterpret_cast<char *>(occ1_in.data()), (std::streamsize)(occ1_in.size() * 4));
        const uint64_t c_occ2 = get_count(in);
        std::vector<uint8_t> occ2_in(c_occ2 * 4);
        in.read(reinterpret_cast<char *>(occ2_in.data()), (std::streamsize)occ2_in.size());
        const uint64_t c_sa = get_count(in);
        if (c_sa != (N + sa_intv - 1) / sa_intv)
            throw std::runtime_error("sa_ of the .fmi does not fit --sa-intv " + std::to_string(sa_intv));
        std::vector<uint32_t> sa_in(c_sa);
        in.read(reinterpret_cast<char *>(sa_in.data()), (std::streamsize)(c_sa * 4));
        const uint64_t c_lookup = get_count(in);
        lookup_len = 0;
        while (lookup_len <= KISS_HIP_FMI_MAX_LOOKUP_LEN && (1ull << (2 * lookup_len)) + 1 != c_lookup) lookup_len++;
        if (lookup_len > KISS_HIP_FMI_MAX_LOOKUP_LEN) throw std::runtime_error("bad lookup size in .fmi (not 4^L + 1)");
        alloc(N - 1);
        if (c_occ1 * 4 != z.occ1_entries) throw std::runtime_error("bad occ1 size in .fmi");
        if (c_occ2 * 4 != z.occ2_bytes) throw std::runtime_error("bad occ2 size in .fmi");
        bwt.swap(bwt_in);
        occ1.swap(occ1_in);
        occ2.swap(occ2_in);
        sa.swap(sa_in);
        in.read(reinterpret_cast<char *>(lookup.data()), (std::streamsize)(c_lookup * 4));
        if (sa_intv != 1) {
            if (get_count(in) != N) throw std::runtime_error("bad b_ size in .fmi");
            in.read(reinterpret_cast<char *>(b.data()), (std::streamsize)(z.b_words * 8));
            if (get_count(in) != z.b_occ_entries) throw std::runtime_error("bad b_occ_ size in .fmi");
            in.read(reinterpret_cast<char *>(b_occ.data()), (std::streamsize)(z.b_occ_entries * 4));
        }
        if (!in || in.peek() != EOF) throw std::runtime_error("trailing or missing bytes in .fmi"); // fm_index.hpp:642
    }
    kiss_hip_fmi_view view() const
    {
        kiss_hip_fmi_view v{};
        v.n_sa = z.n_sa;
        for (int c = 0; c < 4; c++) v.cnt[c] = cnt[c];
        v.pri = pri;
        v.sa_intv = sa_intv;
        v.bwt = bwt.data();
        v.occ1 = occ1.data();
        v.occ2 = occ2.data();
        v.sa = sa.data();
        v.b = sa_intv == 1 ? nullptr : b.data();
        v.b_occ = sa_intv == 1 ? nullptr : b_occ.data();
        return v;
    }
    kiss_hip_fmi_view_ex view_ex() const
    {
        kiss_hip_fmi_view_ex v{};
        v.base = view();
        v.lookup_len = lookup_len;
        v.lookup = lookup.data();
        return v;
    }
    // the batched query of either entry point (host pointers)
    void query(const uint8_t *pat, uint32_t L, uint64_t Q, uint32_t *beg, uint32_t *end, uint64_t *hits, uint64_t *chk,
               uint32_t *offsets, uint64_t *offsets_index, uint64_t capacity, int device) const
    {
        if (classic()) {
            const kiss_hip_fmi_view v = view();
            check(kiss_hip_fmi_query_batch_host(&v, pat, L, Q, beg, end, hits, chk, offsets, offsets_index, capacity, device),
                  "kiss_hip_fmi_query_batch_host");
        } else {
            const kiss_hip_fmi_view_ex v = view_ex();
            check(kiss_hip_fmi_query_ex_host(&v, pat, L, Q, 0, beg, end, nullptr, hits, chk, offsets, offsets_index, capacity,
                                             device),
                  "kiss_hip_fmi_query_ex_host");
        }
    }
};

// bases of a FASTA / plain-text file by the device parser's rule (fasta.hip) -- on the host, without a device, so that
// --output-lcp with a bounded k is decided before anything else happens.  FASTA iff the first byte is '>'; there a line
// that BEGINS with '>' is a header unless the line before it was one (the line after a header is always sequence: in a
// run of '>' lines the 1st, 3rd, ... are headers); every byte of the other lines except '\n' is a base.
uint64_t count_bases_host(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    std::vector<char> buf(1 << 20);
    uint64_t n = 0;
    bool first = true, fasta = false, line_start = true, header = false, prev_header = false;
    while (in) {
        in.read(buf.data(), (std::streamsize)buf.size());
        const std::streamsize got = in.gcount();
        for (std::streamsize i = 0; i < got; i++) {
            const char c = buf[(size_t)i];
            if (first) {
                fasta = c == '>';
                first = false;
            }
            if (line_start) {
                header = fasta && c == '>' && !prev_header;
                line_start = false;
            }
            if (c == '\n') {
                prev_header = header;
                header = false;
                line_start = true;
            } else if (!header) {
                n++;
            }
        }
    }
    return n;
}

// --output-lcp needs the exact order: k = -1 or k >= n (n bounded by the file size first, counted only when that does not decide)
[[noreturn]] void refuse_lcp(long long k)
{
    throw std::runtime_error("--output-lcp needs the exact suffix array: sort with -k -1 (k = " + std::to_string(k) +
                             " is shorter than the text; the LCP array of a k-ordered suffix array is not defined)");
}
void check_lcp_request(const Args &a)
{
    if (a.output_lcp.empty()) return;
    if (a.devices.size() > 1) throw std::runtime_error("--output-lcp: one device only (not with --gpus / --devices)");
    if (a.k < 0) return;
    uint64_t bytes = 0;
    if (kiss_hip_file_size(a.fasta.c_str(), &bytes) != KISS_HIP_OK) throw std::runtime_error("cannot open " + a.fasta);
    if ((uint64_t)a.k >= bytes || (uint64_t)a.k >= count_bases_host(a.fasta)) return;
    refuse_lcp(a.k);
}

int suffix_sort_main(const Args &a)
{
    check_lcp_request(a); // (before any device work)
    const bool multi = a.devices.size() > 1;
    kiss_hip_multi *mc = nullptr;
    double multi_create_s = 0;
    if (multi) { // one process, several devices: the per-device contexts come first, the first one also loads the file
        // Two distinct GPUs exchange the whole LMS list and gather half of the sorted list over the ONE xGMI link between
        // them: the phase model (bench.py: scaling_model) puts a chm13-size sort at about 97 ms on two GPUs
        // against 80 ms on one.  The result is the same; the user is told that the second GPU does not pay.
        if (a.devices.size() == 2 && a.devices[0] != a.devices[1])
            std::fprintf(stderr, "[warning] --gpus 2: two GPUs share one xGMI link for the exchange of the LMS list and the gather of the "
                                 "sorted pieces; the phase model expects this to be SLOWER than one GPU (about 0.8x; 4 GPUs: about "
                                 "1.4x, 8 GPUs: about 2.1x).  Same result either way.\n");
        uint64_t bytes = 0;
        if (kiss_hip_file_size(a.fasta.c_str(), &bytes) != KISS_HIP_OK) throw std::runtime_error("cannot open " + a.fasta);
        const auto tc = std::chrono::steady_clock::now();
        check(kiss_hip_multi_create(&mc, a.devices.data(), (int)a.devices.size(), bytes ? bytes : 1), "kiss_hip_multi_create");
        multi_create_s = seconds_since(tc);
    }
    struct McGuard {
        kiss_hip_multi *&m;
        ~McGuard()
        {
            if (m) kiss_hip_multi_destroy(m);
        }
    } mc_guard{mc};
    DeviceText T(a.fasta, a.device, multi ? kiss_hip_multi_ctx(mc, 0) : nullptr);
    int algo;
    if (a.algo == "PARALLEL_SORTING") algo = KISS_HIP_ALGO_PARALLEL_SORTING;
    else if (a.algo == "PREFIX_DOUBLING") algo = KISS_HIP_ALGO_PREFIX_DOUBLING;
    else throw std::invalid_argument("Invalid sorting algorithm");
    const uint32_t k = (uint32_t)(uint64_t)a.k; // -1 -> size_t max -> truncated to 0xFFFFFFFF (suffix_sort.hpp:35-37)
    if (!a.output_lcp.empty() && a.k >= 0 && (uint64_t)a.k < T.n) refuse_lcp(a.k); // (the parsed n: still before the sort)
    void *d_SA = nullptr;
    const auto ta = std::chrono::steady_clock::now();
    check(kiss_hip_alloc_dev(&d_SA, (T.n + 1) * sizeof(uint32_t)), "kiss_hip_alloc_dev");
    const double alloc_s = seconds_since(ta);
    const auto t0 = std::chrono::steady_clock::now(); // the reference starts its stopwatch here (suffix_sort.hpp:57)
    if (multi)
        check(kiss_hip_multi_suffix_sort_dna_u32_dev(mc, T.d_S, T.n, k, algo, (uint32_t *)d_SA),
              "kiss_hip_multi_suffix_sort_dna_u32_dev");
    else
        check(kiss_hip_ctx_suffix_sort_dna_u32_dev(T.ctx, T.d_S, T.n, k, algo, (uint32_t *)d_SA, nullptr),
              "kiss_hip_ctx_suffix_sort_dna_u32_dev");
    const double el = seconds_since(t0);
    std::fprintf(stderr, "[info] n = %llu, k = %llu, suffix sorting elapsed %.6f\n", (unsigned long long)T.n,
                 (unsigned long long)(a.k < 0 ? ~0ull : (unsigned long long)a.k), el);
    if (multi && a.verbose) {
        kiss_hip_multi_stats ms;
        kiss_hip_multi_get_stats(mc, &ms);
        std::fprintf(stderr, "[debug] %u devices (workspaces %.6f s): pack + broadcast %.3f ms, get_lms per slice %.3f ms, "
                             "partition %.3f ms, exchange %.3f ms, lms_suffix_direct_sort per key range %.3f ms, gather %.3f ms, "
                             "put_lms_suffix + induced_sort %.3f ms, total %.3f ms; lms = %llu\n",
                     ms.ndev, multi_create_s, ms.ms_pack, ms.ms_classify, ms.ms_partition, ms.ms_exchange, ms.ms_sort,
                     ms.ms_gather, ms.ms_induce, ms.ms_total, (unsigned long long)ms.m);
    }
    if (!multi && a.verbose) {
        kiss_hip_stats st;
        kiss_hip_get_stats(T.ctx, &st);
        std::fprintf(stderr, "[debug] device workspace %.6f s; read + upload + device-side parse of %s %.6f s; SA buffer %.6f s\n",
                     T.create_s, a.fasta.c_str(), T.load_s, alloc_s);
        std::fprintf(stderr,
                     "[debug] device: pack %.3f ms, get_lms %.3f ms, lms_suffix_direct_sort %.3f ms, put_lms_suffix %.3f ms, "
                     "induced_sort %.3f ms, prefix_doubling %.3f ms, total %.3f ms; lms = %llu, rounds = %u + %u, passes = %u\n",
                     st.ms_pack, st.ms_classify, st.ms_lms_sort, st.ms_place, st.ms_induce, st.ms_refine, st.ms_total,
                     (unsigned long long)st.m, st.lms_rounds, st.doubling_rounds, st.induce_passes);
    }
    if (!a.output_sa.empty()) write_dev_u32(a.output_sa, d_SA, T.n + 1);
    if (!a.output_lcp.empty()) { // in place: the SA buffer becomes the LCP array
        kiss_hip_lcp_report rep{};
        const auto tl = std::chrono::steady_clock::now();
        check(kiss_hip_ctx_lcp_dna_u32_dev(T.ctx, T.d_S, T.n, (const uint32_t *)d_SA, (uint32_t *)d_SA, &rep, nullptr),
              "kiss_hip_ctx_lcp_dna_u32_dev");
        std::fprintf(stderr, "[info] LCP array elapsed %.6f (device %.3f ms: phi %.3f, short %.3f, long %.3f, scan + gather %.3f; "
                             "irreducible %llu, long pairs %llu, max lcp %u)\n",
                     seconds_since(tl), rep.ms_total, rep.ms_phi, rep.ms_short, rep.ms_long, rep.ms_scan_gather,
                     (unsigned long long)rep.irreducible, (unsigned long long)rep.long_pairs, rep.max_lcp);
        write_dev_u32(a.output_lcp, d_SA, T.n + 1);
    }
    const auto tf = std::chrono::steady_clock::now();
    kiss_hip_free_dev(d_SA);
    if (a.verbose) std::fprintf(stderr, "[debug] SA buffer released in %.6f s\n", seconds_since(tf));
    return 0;
}

int fmindex_build_main(const Args &a)
{
    std::vector<uint8_t> S;
    {
        DeviceText T(a.fasta, a.device);
        S = T.to_host();
    }
    if (S.empty()) throw std::runtime_error("empty sequence");
    Fmi f(a.sa_intv, a.lookup_len);
    f.alloc(S.size());
    std::vector<uint32_t> SA; // --exact: the exact suffix array instead of the build's own k = 32 sort
    if (a.exact) {
        SA.resize(S.size() + 1);
        check(kiss_hip_suffix_sort_dna_u32(S.data(), S.size(), 0xFFFFFFFFu, KISS_HIP_ALGO_PARALLEL_SORTING, SA.data(), a.device),
              "kiss_hip_suffix_sort_dna_u32");
    }
    const uint32_t *sa_or_null = a.exact ? SA.data() : nullptr;
    if (f.classic())
        check(kiss_hip_fmi_build_host(S.data(), S.size(), sa_or_null, f.bwt.data(), f.occ1.data(), f.occ2.data(), f.sa.data(),
                                      f.b.data(), f.b_occ.data(), f.cnt, &f.pri, a.device),
              "kiss_hip_fmi_build_host");
    else
        check(kiss_hip_fmi_build_ex_host(S.data(), S.size(), sa_or_null, f.sa_intv, f.lookup_len, f.bwt.data(), f.occ1.data(),
                                         f.occ2.data(), f.sa.data(), f.b.data(), f.b_occ.data(), f.lookup.data(), f.cnt,
                                         &f.pri, a.device),
              "kiss_hip_fmi_build_ex_host");
    f.save(a.fasta + ".fmi");
    return 0;
}

const char *ending(size_t x)
{
    x %= 100;
    if (x / 10 == 1) return "th";
    if (x % 10 == 1) return "st";
    if (x % 10 == 2) return "nd";
    if (x % 10 == 3) return "rd";
    return "th";
}

// fmindex_query --mismatches: counts first (they size the output), then the hits of every pattern in ascending position
struct MmHits {
    std::vector<uint32_t> counts, positions;
    std::vector<uint8_t> mismatches;
    std::vector<uint64_t> index;
    kiss_hip_fmi_mm_report rep{};
    uint64_t total = 0;
};
MmHits mm_query(const Fmi &f, const uint8_t *pat, uint32_t L, uint64_t Q, uint32_t e, int device)
{
    MmHits h;
    const kiss_hip_fmi_view v = f.view();
    h.counts.resize((size_t)Q * (e + 1) + 1);
    check(kiss_hip_fmi_query_mm_host(&v, pat, L, Q, e, h.counts.data(), nullptr, nullptr, nullptr, 0, &h.rep, device),
          "kiss_hip_fmi_query_mm_host");
    for (int j = 0; j < 4; j++) h.total += h.rep.hits[j];
    h.positions.resize(h.total + 1);
    h.mismatches.resize(h.total + 1);
    h.index.resize(Q + 1);
    const int rc = kiss_hip_fmi_query_mm_host(&v, pat, L, Q, e, h.counts.data(), h.positions.data(), h.mismatches.data(),
                                              h.index.data(), h.total, &h.rep, device);
    if (rc == KISS_HIP_E_INVALID && h.rep.walk_failures)
        throw std::runtime_error("fmindex_query --mismatches: " + std::to_string(h.rep.walk_failures) +
                                 " rows of the index reached no sampled row: the positions need an index built with "
                                 "fmindex_build --exact");
    check(rc, "kiss_hip_fmi_query_mm_host");
    return h;
}

// The records of the reference file, scanned on the host under the parse rules of fasta.hip: the file is FASTA iff its first
// byte is '>'; a line that begins with '>' is a header unless the line in front of it was one (the line after a header is
// always sequence); every byte of a sequence line except '\n' is a base.  A plain-text file is one record named after the
// file.  Records without bases are left out (SAM has no LN:0, and the record starts must ascend strictly).
struct RefRecords {
    std::vector<std::string> names;
    std::vector<uint64_t> bounds{0};
};
RefRecords scan_records(const std::string &path)
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
    const int first = in.peek();
    const bool fasta = first == '>';
    bool after_header = false;
    std::string line;
    while (std::getline(in, line)) {
        if (fasta && !after_header && !line.empty() && line[0] == '>') {
            close();
            const size_t ws = line.find_first_of(" \t\r", 1);
            name = line.substr(1, ws == std::string::npos ? std::string::npos : ws - 1);
            after_header = true;
            continue;
        }
        after_header = false;
        len += line.size();
    }
    close();
    return r;
}

// --rescue: what the second pass needs to know of the first -- the source of every merged alignment (below first_alns: a read's
// own), the first pass's pairs and the plan's report
struct Rescued {
    std::vector<uint32_t> source;
    uint64_t first_alns = 0;
    std::vector<kiss_hip_pair> first_pairs;
    kiss_hip_rescue_report plan{};
};

// fmindex_query --seeds READS --mates READS2 --chain --align --sam: the hits of reads 2 p and 2 p + 1 paired, the body of the SAM
// (out: the header).  The lines of mate 1, then those of mate 2; of a mate its chosen hit first -- without 256 / 2048, with the
// pair's MAPQ, signed TLEN, YS:i: (the mate's score) and, in a proper pair, YT:Z:CP --, then its other hits in hit order with their
// own flags and MAPQ (a hit number 0 that was not chosen: 256 and MAPQ 0) and TLEN 0.  Every line carries 1, 64 / 128, 8 / 32 for
// the mate, and RNEXT / PNEXT of the mate's chosen hit; a mate that did not map lies where its partner does (SAM's convention).
int sam_pairs(const Args &a, std::string &out, const RefRecords &ref, const std::vector<kiss_hip_aln> &alns, const std::vector<uint32_t> &cigar,
              const std::vector<uint64_t> &oidx, const std::vector<uint8_t> &reads, const std::vector<uint64_t> &ridx,
              const std::vector<std::string> &names, const std::vector<kiss_hip_hit> &hits, const std::vector<uint64_t> &hidx,
              const kiss_hip_select_report &srep, const Rescued *rescued = nullptr)
{
    const uint64_t Q = ridx.size() - 1, P = Q / 2, R = ref.names.size();
    std::vector<kiss_hip_pair> pairs(P + 1);
    kiss_hip_pair_report rep{};
    check(kiss_hip_fmi_pair_host(hits.data(), hidx.data(), Q, alns.data(), srep.alignments, &a.pair_params, pairs.data(), &rep, a.device),
          "kiss_hip_fmi_pair_host");
    for (uint64_t p = 0; p < P; p++) {
        const kiss_hip_pair &pr = pairs[p];
        if (pr.flags & KISS_HIP_PAIR_BAD_INPUT) throw std::runtime_error("kiss_hip_fmi_pair_host: pair " + std::to_string(p) + " is bad input");
        const uint32_t chosen[2] = {pr.hit1, pr.hit2}, mapq[2] = {pr.mapq1, pr.mapq2};
        const bool proper = (pr.flags & KISS_HIP_PAIR_PROPER) != 0;
        // where a mate lies: its chosen hit
        bool mapped[2], rev[2] = {false, false};
        std::string rname[2] = {"*", "*"};
        uint64_t pos[2] = {0, 0}, tbeg[2] = {0, 0};
        for (int m = 0; m < 2; m++) {
            mapped[m] = chosen[m] != KISS_HIP_PAIR_NONE;
            if (!mapped[m]) continue;
            const kiss_hip_hit &t = hits[chosen[m]];
            rev[m] = (t.flags & KISS_HIP_HIT_REVERSE) != 0;
            if (R) rname[m] = ref.names[t.ref];
            tbeg[m] = alns[t.aln].tbeg;
            pos[m] = tbeg[m] - (R ? ref.bounds[t.ref] : 0) + 1;
        }
        for (int m = 0; m < 2; m++) {
            const int o = 1 - m;
            const uint64_t q = 2 * p + (uint64_t)m, L = ridx[q + 1] - ridx[q];
            const auto seq = [&](bool reverse) {
                std::string s(L, 'N');
                for (uint64_t j = 0; j < L; j++) {
                    const uint8_t c = reads[ridx[q] + (reverse ? L - 1 - j : j)];
                    if (c <= 3) s[j] = "ACGT"[reverse ? 3 - c : c];
                }
                return s;
            };
            const unsigned base = 1u | (m ? 128u : 64u) | (mapped[o] ? 0u : 8u) | (mapped[o] && rev[o] ? 32u : 0u);
            if (!mapped[m]) { // at its partner's place, if that has one
                out += names[q] + '\t' + std::to_string(base | 4u) + '\t' + rname[o] + '\t' + std::to_string(pos[o]) + "\t0\t*\t" +
                       (mapped[o] ? "=" : "*") + '\t' + std::to_string(pos[o]) + "\t0\t" + seq(false) + "\t*\n";
                continue;
            }
            // the mate's place, or this read's own when the mate has none
            const std::string &next_name = mapped[o] ? rname[o] : rname[m];
            const uint64_t next_pos = mapped[o] ? pos[o] : pos[m];
            long long tlen = 0;
            if (mapped[o] && pr.tlen) tlen = (tbeg[m] < tbeg[o] || (tbeg[m] == tbeg[o] && m == 0)) ? (long long)pr.tlen : -(long long)pr.tlen;
            const auto line = [&](uint64_t h, bool is_chosen) {
                const kiss_hip_hit &t = hits[h];
                const uint64_t c = t.aln;
                const kiss_hip_aln &k = alns[c];
                const bool reverse = (t.flags & KISS_HIP_HIT_REVERSE) != 0, head = !(t.flags & KISS_HIP_HIT_SECONDARY);
                unsigned flag = base | (reverse ? 16u : 0u);
                uint32_t q_mapq = t.mapq;
                if (is_chosen) {
                    flag |= proper ? 2u : 0u;
                    q_mapq = mapq[m];
                } else {
                    flag |= (t.flags & KISS_HIP_HIT_SECONDARY ? 256u : 0u) | (t.flags & KISS_HIP_HIT_SUPPLEMENTARY ? 2048u : 0u);
                    if (h == hidx[q]) { // the primary of the read on its own, displaced by the pair
                        flag |= 256u;
                        q_mapq = 0;
                    }
                }
                const std::string name = R ? ref.names[t.ref] : std::string("*");
                out += names[q] + '\t' + std::to_string(flag) + '\t' + name + '\t' +
                       std::to_string((uint64_t)k.tbeg - (R ? ref.bounds[t.ref] : 0) + 1) + '\t' + std::to_string(q_mapq) + '\t';
                if (k.rbeg) out += std::to_string(k.rbeg) + 'S';
                for (uint64_t x = oidx[c]; x < oidx[c + 1]; x++) out += std::to_string(cigar[x] >> 4) + "MID"[cigar[x] & 15u];
                if (L > k.rend) out += std::to_string(L - k.rend) + 'S';
                out += '\t' + (name == next_name ? std::string("=") : next_name) + '\t' + std::to_string(next_pos) + '\t' +
                       std::to_string(is_chosen ? tlen : 0ll) + '\t' + seq(reverse) + "\t*\tNM:i:" + std::to_string(k.mismatches + k.ins + k.del) +
                       "\tAS:i:" + std::to_string(t.score);
                if (head) out += "\tXS:i:" + std::to_string(t.sub);
                if (is_chosen && mapped[o]) out += "\tYS:i:" + std::to_string(hits[chosen[o]].score);
                if (is_chosen && proper) out += "\tYT:Z:CP";
                if (rescued && rescued->source[c] >= rescued->first_alns) out += "\tYR:i:1";
                out += '\n';
            };
            line(chosen[m], true);
            for (uint64_t h = hidx[q]; h < hidx[q + 1]; h++)
                if (h != chosen[m]) line(h, false);
        }
        if (out.size() > (1u << 20)) {
            std::fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    std::fprintf(stderr, "[info] reads: %llu, alignments: %llu, candidates: %llu, spanning: %llu, redundant: %llu, hits: %llu, "
                         "heads: %llu, mapped: %llu, most candidates of a read: %u\n",
                 (unsigned long long)Q, (unsigned long long)srep.alignments, (unsigned long long)srep.candidates,
                 (unsigned long long)srep.spanning, (unsigned long long)srep.redundant, (unsigned long long)srep.hits,
                 (unsigned long long)srep.heads, (unsigned long long)srep.mapped, srep.max_candidates);
    std::fprintf(stderr, "[info] pairs: %llu, eligible hits: %llu, combinations: %llu, concordant: %llu, proper: %llu, promoted: %llu, "
                         "lifted: %llu, most combinations of a pair: %llu\n",
                 (unsigned long long)rep.P, (unsigned long long)rep.eligible, (unsigned long long)rep.combinations,
                 (unsigned long long)rep.concordant, (unsigned long long)rep.proper, (unsigned long long)rep.promoted,
                 (unsigned long long)rep.lifted, (unsigned long long)rep.max_combinations);
    if (rescued) {
        uint64_t now_proper = 0;
        for (uint64_t p = 0; p < P; p++)
            now_proper += (pairs[p].flags & KISS_HIP_PAIR_PROPER) && !(rescued->first_pairs[p].flags & KISS_HIP_PAIR_PROPER) ? 1u : 0u;
        const kiss_hip_rescue_report &pl = rescued->plan;
        std::fprintf(stderr, "[info] rescue: pairs planned: %llu, anchors: %llu, chains: %llu, split: %llu, empty: %llu, bad input: %llu, "
                             "most chains of a pair: %llu, rescued: %llu\n",
                     (unsigned long long)pl.pairs_planned, (unsigned long long)pl.anchors, (unsigned long long)pl.chains,
                     (unsigned long long)pl.split, (unsigned long long)pl.empty, (unsigned long long)pl.bad_input,
                     (unsigned long long)pl.max_chains, (unsigned long long)now_proper);
    }
    return 0;
}

// fmindex_query ... --mates READS2 --sam --rescue: the first pass paired, the pairs that are not proper planned into windows
// (kiss_hip_fmi_rescue_host), the windows aligned (the align call as it is), their alignments merged behind the reads' own
// (kiss_hip_fmi_aln_merge_host), the mappings picked again; sam_pairs then pairs and writes the merged set
int sam_rescue(const Args &a, std::string &out, const RefRecords &ref, const std::vector<uint8_t> &S, const std::vector<kiss_hip_aln> &alns,
               const std::vector<uint64_t> &cidx, const std::vector<uint32_t> &cigar, const std::vector<uint64_t> &oidx,
               const std::vector<uint8_t> &reads, const std::vector<uint64_t> &ridx, const std::vector<std::string> &names,
               const std::vector<kiss_hip_hit> &hits, const std::vector<uint64_t> &hidx, const kiss_hip_select_report &srep)
{
    const uint64_t Q = ridx.size() - 1, P = Q / 2, V = 2 * Q, R = ref.names.size(), CA = srep.alignments, n = S.size();
    const uint64_t *bounds = R ? ref.bounds.data() : nullptr;
    Rescued rs;
    rs.first_alns = CA;
    rs.first_pairs.resize(P + 1);
    check(kiss_hip_fmi_pair_host(hits.data(), hidx.data(), Q, alns.data(), CA, &a.pair_params, rs.first_pairs.data(), nullptr, a.device),
          "kiss_hip_fmi_pair_host");
    // the plan: the first call sizes the chains
    std::vector<kiss_hip_chain> chains(1);
    std::vector<uint64_t> rcidx(V + 1, 0);
    int rc = kiss_hip_fmi_rescue_host(rs.first_pairs.data(), hits.data(), hidx.data(), Q, alns.data(), CA, ridx.data(), n, bounds, R,
                                      &a.rescue_params, chains.data(), rcidx.data(), nullptr, 0, &rs.plan, a.device);
    if (rc == KISS_HIP_E_INVALID && rs.plan.chains) {
        chains.resize(rs.plan.chains);
        rc = kiss_hip_fmi_rescue_host(rs.first_pairs.data(), hits.data(), hidx.data(), Q, alns.data(), CA, ridx.data(), n, bounds, R,
                                      &a.rescue_params, chains.data(), rcidx.data(), nullptr, rs.plan.chains, &rs.plan, a.device);
    }
    check(rc, "kiss_hip_fmi_rescue_host");
    const uint64_t CB = rs.plan.chains;
    // the windows aligned: the first call sizes the ops
    std::vector<kiss_hip_aln> ralns(CB + 1);
    std::vector<uint32_t> rcigar(1);
    std::vector<uint64_t> roidx(CB + 1, 0);
    kiss_hip_align_report arep{};
    rc = kiss_hip_fmi_align_host(S.data(), n, reads.data(), ridx.data(), Q, 1, chains.data(), rcidx.data(), &a.align_params, ralns.data(), CB,
                                 rcigar.data(), roidx.data(), 0, &arep, a.device);
    if (rc == KISS_HIP_E_INVALID && arep.cigar_ops) {
        rcigar.resize(arep.cigar_ops);
        rc = kiss_hip_fmi_align_host(S.data(), n, reads.data(), ridx.data(), Q, 1, chains.data(), rcidx.data(), &a.align_params, ralns.data(),
                                     CB, rcigar.data(), roidx.data(), arep.cigar_ops, &arep, a.device);
    }
    if (rc == KISS_HIP_E_UNSUPPORTED && arep.cells)
        throw std::runtime_error("fmindex_query --rescue: " + std::to_string(arep.cells) +
                                 " DP cells are more than one call holds: split the reads");
    check(rc, "kiss_hip_fmi_align_host");
    // merged: capacities are known
    const uint64_t C = CA + CB, ops = oidx[CA] + roidx[CB];
    std::vector<kiss_hip_aln> malns(C + 1);
    std::vector<uint64_t> mcidx(V + 1, 0), moidx(C + 1, 0);
    std::vector<uint32_t> mcigar(ops + 1);
    rs.source.resize(C + 1);
    check(kiss_hip_fmi_aln_merge_host(alns.data(), cidx.data(), cigar.data(), oidx.data(), ralns.data(), rcidx.data(), rcigar.data(),
                                      roidx.data(), V, malns.data(), C, mcidx.data(), rs.source.data(), mcigar.data(), moidx.data(), ops,
                                      nullptr, a.device),
          "kiss_hip_fmi_aln_merge_host");
    std::vector<kiss_hip_hit> mhits(C + 1);
    std::vector<uint64_t> mhidx(Q + 1, 0);
    kiss_hip_select_report rep{};
    check(kiss_hip_fmi_select_host(malns.data(), mcidx.data(), ridx.data(), Q, 1, bounds, R, &a.select_params, mhits.data(), mhidx.data(), C,
                                   &rep, a.device),
          "kiss_hip_fmi_select_host");
    return sam_pairs(a, out, ref, malns, mcigar, moidx, reads, ridx, names, mhits, mhidx, rep, &rs);
}

// fmindex_query --seeds READS --chain --align --sam: the alignments of every read turned into its mappings, stdout is SAM
int sam_main(const Args &a, uint64_t C, const std::vector<uint8_t> &S, const std::vector<kiss_hip_aln> &alns, const std::vector<uint64_t> &cidx,
             const std::vector<uint32_t> &cigar, const std::vector<uint64_t> &oidx, const std::vector<uint8_t> &reads,
             const std::vector<uint64_t> &ridx, const std::vector<std::string> &names)
{
    const uint64_t n = S.size();
    const uint64_t Q = ridx.size() - 1;
    const RefRecords ref = scan_records(a.fasta);
    if (ref.bounds.back() != n)
        throw std::runtime_error("fmindex_query --sam: the records of " + a.fasta + " have " + std::to_string(ref.bounds.back()) +
                                 " bases, the parsed text has " + std::to_string(n));
    const uint64_t R = ref.names.size();
    std::vector<kiss_hip_hit> hits(C + 1); // (a read keeps no more hits than it has alignments: one call)
    std::vector<uint64_t> hidx(Q + 1, 0);
    kiss_hip_select_report rep{};
    check(kiss_hip_fmi_select_host(alns.data(), cidx.data(), ridx.data(), Q, a.both_strands, R ? ref.bounds.data() : nullptr, R,
                                   &a.select_params, hits.data(), hidx.data(), C, &rep, a.device),
          "kiss_hip_fmi_select_host");
    std::string out = "@HD\tVN:1.6\tSO:unsorted\n";
    for (uint64_t r = 0; r < R; r++)
        out += "@SQ\tSN:" + ref.names[r] + "\tLN:" + std::to_string(ref.bounds[r + 1] - ref.bounds[r]) + '\n';
    out += std::string("@PG\tID:kiss\tPN:kiss\tVN:") + VERSION + '\n';
    if (a.rescue) return sam_rescue(a, out, ref, S, alns, cidx, cigar, oidx, reads, ridx, names, hits, hidx, rep);
    if (!a.mates.empty()) return sam_pairs(a, out, ref, alns, cigar, oidx, reads, ridx, names, hits, hidx, rep);
    for (uint64_t q = 0; q < Q; q++) {
        const uint64_t L = ridx[q + 1] - ridx[q];
        const auto seq = [&](bool reverse) {
            std::string s(L, 'N');
            for (uint64_t j = 0; j < L; j++) {
                const uint8_t c = reads[ridx[q] + (reverse ? L - 1 - j : j)];
                if (c <= 3) s[j] = "ACGT"[reverse ? 3 - c : c];
            }
            return s;
        };
        if (hidx[q + 1] == hidx[q]) {
            out += names[q] + "\t4\t*\t0\t0\t*\t*\t0\t0\t" + seq(false) + "\t*\n";
            continue;
        }
        for (uint64_t h = hidx[q]; h < hidx[q + 1]; h++) {
            const kiss_hip_hit &t = hits[h];
            const uint64_t c = t.aln; // (alignment a: alns[a] and the ops oidx[a] .. oidx[a + 1])
            const kiss_hip_aln &k = alns[c];
            const bool reverse = (t.flags & KISS_HIP_HIT_REVERSE) != 0, head = !(t.flags & KISS_HIP_HIT_SECONDARY);
            const unsigned flag = (reverse ? 16u : 0u) | (t.flags & KISS_HIP_HIT_SECONDARY ? 256u : 0u) |
                                  (t.flags & KISS_HIP_HIT_SUPPLEMENTARY ? 2048u : 0u);
            out += names[q] + '\t' + std::to_string(flag) + '\t' + (R ? ref.names[t.ref] : std::string("*")) + '\t' +
                   std::to_string((uint64_t)k.tbeg - (R ? ref.bounds[t.ref] : 0) + 1) + '\t' + std::to_string(t.mapq) + '\t';
            if (k.rbeg) out += std::to_string(k.rbeg) + 'S';
            for (uint64_t o = oidx[c]; o < oidx[c + 1]; o++) out += std::to_string(cigar[o] >> 4) + "MID"[cigar[o] & 15u];
            if (L > k.rend) out += std::to_string(L - k.rend) + 'S';
            out += "\t*\t0\t0\t" + seq(reverse) + "\t*\tNM:i:" + std::to_string(k.mismatches + k.ins + k.del) + "\tAS:i:" +
                   std::to_string(t.score);
            if (head) out += "\tXS:i:" + std::to_string(t.sub);
            out += '\n';
        }
        if (out.size() > (1u << 20)) {
            std::fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    std::fprintf(stderr, "[info] reads: %llu, alignments: %llu, candidates: %llu, spanning: %llu, redundant: %llu, hits: %llu, "
                         "heads: %llu, mapped: %llu, most candidates of a read: %u\n",
                 (unsigned long long)Q, (unsigned long long)rep.alignments, (unsigned long long)rep.candidates,
                 (unsigned long long)rep.spanning, (unsigned long long)rep.redundant, (unsigned long long)rep.hits,
                 (unsigned long long)rep.heads, (unsigned long long)rep.mapped, rep.max_candidates);
    return 0;
}

// fmindex_query --seeds READS --chain --align: one line per chain on stdout, `read strand score rbeg rend tbeg tend nm cigar`
int align_main(const Args &a, uint64_t V, const std::vector<kiss_hip_chain> &chains, const std::vector<uint64_t> &cidx,
               const std::vector<uint8_t> &reads, const std::vector<uint64_t> &ridx, const std::vector<std::string> &names)
{
    std::vector<uint8_t> S;
    {
        DeviceText T(a.fasta, a.device);
        S = T.to_host();
    }
    S.reserve(1); // (a pointer that is not NULL)
    const uint64_t Q = ridx.size() - 1, C = cidx[V], n = S.size();
    std::vector<kiss_hip_aln> alns(C + 1);
    std::vector<uint32_t> cigar(1);
    std::vector<uint64_t> oidx(C + 1, 0);
    kiss_hip_align_report rep{};
    // the first call sizes the ops
    int rc = kiss_hip_fmi_align_host(S.data(), n, reads.data(), ridx.data(), Q, a.both_strands, chains.data(), cidx.data(),
                                     &a.align_params, alns.data(), C, cigar.data(), oidx.data(), 0, &rep, a.device);
    if (rc == KISS_HIP_E_INVALID && rep.cigar_ops) {
        cigar.resize(rep.cigar_ops);
        rc = kiss_hip_fmi_align_host(S.data(), n, reads.data(), ridx.data(), Q, a.both_strands, chains.data(), cidx.data(),
                                     &a.align_params, alns.data(), C, cigar.data(), oidx.data(), rep.cigar_ops, &rep, a.device);
    }
    if (rc == KISS_HIP_E_UNSUPPORTED && rep.cells)
        throw std::runtime_error("fmindex_query --align: " + std::to_string(rep.cells) +
                                 " DP cells are more than one call holds: split the reads");
    check(rc, "kiss_hip_fmi_align_host");
    if (a.sam) return sam_main(a, C, S, alns, cidx, cigar, oidx, reads, ridx, names);
    std::string out;
    for (uint64_t vr = 0; vr < V; vr++) {
        const uint64_t q = a.both_strands ? vr / 2 : vr, L = ridx[q + 1] - ridx[q];
        const char strand = a.both_strands && (vr & 1) ? '-' : '+';
        for (uint64_t c = cidx[vr]; c < cidx[vr + 1]; c++) {
            const kiss_hip_aln &k = alns[c];
            out += std::to_string(q) + ' ' + strand + ' ' + std::to_string(k.score) + ' ' + std::to_string(k.rbeg) + ' ' +
                   std::to_string(k.rend) + ' ' + std::to_string(k.tbeg) + ' ' + std::to_string(k.tend) + ' ' +
                   std::to_string(k.mismatches + k.ins + k.del) + ' ';
            if (oidx[c + 1] == oidx[c]) {
                out += '*';
            } else {
                if (k.rbeg) out += std::to_string(k.rbeg) + 'S';
                for (uint64_t o = oidx[c]; o < oidx[c + 1]; o++) out += std::to_string(cigar[o] >> 4) + "MID"[cigar[o] & 15u];
                if (L > k.rend) out += std::to_string(L - k.rend) + 'S';
            }
            out += '\n';
        }
        if (out.size() > (1u << 20)) {
            std::fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    std::fprintf(stderr, "[info] virtual reads: %llu, chains: %llu, aligned: %llu, band too wide: %llu, best score: %u\n",
                 (unsigned long long)V, (unsigned long long)rep.chains, (unsigned long long)rep.aligned,
                 (unsigned long long)rep.too_wide, rep.best_score);
    return 0;
}

// fmindex_query --seeds READS --chain: one line per chain on stdout, `read strand score anchors rbeg rend tbeg tend`
// (with --align: `read strand score rbeg rend tbeg tend nm cigar`, the fields of the alignment of the chain)
int chains_main(const Args &a, uint64_t V, const std::vector<kiss_hip_fmi_seed> &seeds, const std::vector<uint64_t> &sidx,
                const std::vector<uint32_t> &pos, const std::vector<uint64_t> &pidx, const std::vector<uint8_t> &reads,
                const std::vector<uint64_t> &ridx, const std::vector<std::string> &names)
{
    std::vector<kiss_hip_chain> chains(1);
    std::vector<uint64_t> cidx(V + 1, 0);
    kiss_hip_chain_report rep{};
    // the first call sizes the output
    int rc = kiss_hip_fmi_chain_host(seeds.data(), sidx.data(), V, pos.data(), pidx.data(), &a.chain_params, chains.data(),
                                     cidx.data(), 0, nullptr, nullptr, 0, &rep, a.device);
    if (rc == KISS_HIP_E_INVALID && rep.chains) {
        chains.resize(rep.chains);
        rc = kiss_hip_fmi_chain_host(seeds.data(), sidx.data(), V, pos.data(), pidx.data(), &a.chain_params, chains.data(),
                                     cidx.data(), rep.chains, nullptr, nullptr, 0, &rep, a.device);
    }
    check(rc, "kiss_hip_fmi_chain_host");
    if (a.align) return align_main(a, V, chains, cidx, reads, ridx, names);
    std::string out;
    for (uint64_t vr = 0; vr < V; vr++) {
        const uint64_t q = a.both_strands ? vr / 2 : vr;
        const char strand = a.both_strands && (vr & 1) ? '-' : '+';
        for (uint64_t c = cidx[vr]; c < cidx[vr + 1]; c++) {
            const kiss_hip_chain &k = chains[c];
            out += std::to_string(q) + ' ' + strand + ' ' + std::to_string(k.score) + ' ' + std::to_string(k.anchors) + ' ' +
                   std::to_string(k.rbeg) + ' ' + std::to_string(k.rend) + ' ' + std::to_string(k.tbeg) + ' ' +
                   std::to_string(k.tend) + '\n';
        }
        if (out.size() > (1u << 20)) {
            std::fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    std::fprintf(stderr, "[info] virtual reads: %llu, anchors: %llu, chains: %llu, best score: %u\n", (unsigned long long)V,
                 (unsigned long long)rep.anchors, (unsigned long long)rep.chains, rep.best_score);
    return 0;
}

// fmindex_query --seeds: one line per seed on stdout, `read strand start len count pos...`
int seeds_main(const Args &a, const Fmi &f)
{
    // one file of reads: the codes of its reads one after the other, where they start, and their names
    struct ReadFile {
        std::vector<uint8_t> reads;
        std::vector<uint64_t> ridx{0};
        std::vector<std::string> names; // --sam: the word after '>' on the line directly in front of a read, else its number
    };
    const auto load = [&](const std::string &path) {
        std::ifstream in(path);
        if (!in) throw std::runtime_error("cannot open " + path);
        ReadFile f;
        std::string line, pending;
        while (std::getline(in, line)) {
            if (!line.empty() && line.back() == '\r') line.pop_back();
            if (line.empty() || line[0] == '>') {
                if (a.sam) {
                    const size_t ws = line.find_first_of(" \t", 1);
                    pending = line.empty() ? std::string() : line.substr(1, ws == std::string::npos ? std::string::npos : ws - 1);
                }
                continue;
            }
            if (a.sam) f.names.push_back(pending.empty() ? std::to_string(f.ridx.size() - 1) : pending);
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
    };
    ReadFile one = load(a.seeds);
    if (!a.mates.empty()) { // reads 2 p and 2 p + 1 of the batch are read p of either file
        const ReadFile first = std::move(one), second = load(a.mates);
        const uint64_t P = first.ridx.size() - 1;
        if (second.ridx.size() - 1 != P)
            throw std::runtime_error("fmindex_query --mates: " + a.seeds + " has " + std::to_string(P) + " reads, " + a.mates + " has " +
                                     std::to_string(second.ridx.size() - 1) + " reads: a pair has one of each");
        one = ReadFile();
        for (uint64_t p = 0; p < P; p++)
            for (const ReadFile *f : {&first, &second}) {
                one.reads.insert(one.reads.end(), f->reads.begin() + (std::ptrdiff_t)f->ridx[p], f->reads.begin() + (std::ptrdiff_t)f->ridx[p + 1]);
                one.ridx.push_back(one.reads.size());
                one.names.push_back(f->names[p]);
            }
    }
    const std::vector<uint8_t> &reads = one.reads;
    const std::vector<uint64_t> &ridx = one.ridx;
    const std::vector<std::string> &names = one.names;
    const uint64_t Q = ridx.size() - 1, bases = (a.both_strands ? 2 : 1) * (uint64_t)reads.size();
    const uint64_t V = a.both_strands ? 2 * Q : Q;
    const kiss_hip_fmi_view_ex v = f.view_ex();
    std::vector<kiss_hip_fmi_seed> seeds(bases + 1);
    std::vector<uint64_t> sidx(V + 1, 0), pidx;
    std::vector<uint32_t> pos;
    kiss_hip_fmi_seed_report rep{};
    // the first call sizes the output
    check(kiss_hip_fmi_seeds_host(&v, reads.data(), ridx.data(), Q, a.min_seed_len, a.max_seed_len, a.max_occ, a.both_strands,
                                  nullptr, seeds.data(), sidx.data(), bases, nullptr, nullptr, 0, &rep, a.device),
          "kiss_hip_fmi_seeds_host");
    pos.resize(rep.positions + 1);
    pidx.resize(rep.seeds + 1);
    const int rc = kiss_hip_fmi_seeds_host(&v, reads.data(), ridx.data(), Q, a.min_seed_len, a.max_seed_len, a.max_occ,
                                           a.both_strands, nullptr, seeds.data(), sidx.data(), bases, pos.data(), pidx.data(),
                                           rep.positions, &rep, a.device);
    if (rc == KISS_HIP_E_INVALID && rep.walk_failures)
        throw std::runtime_error("fmindex_query --seeds: " + std::to_string(rep.walk_failures) +
                                 " rows of the index reached no sampled row: the positions need an index built with "
                                 "fmindex_build --exact");
    check(rc, "kiss_hip_fmi_seeds_host");
    if (a.chain) return chains_main(a, V, seeds, sidx, pos, pidx, reads, ridx, names);
    std::string out;
    for (uint64_t vr = 0; vr < V; vr++) {
        const uint64_t q = a.both_strands ? vr / 2 : vr;
        const char strand = a.both_strands && (vr & 1) ? '-' : '+';
        for (uint64_t s = sidx[vr]; s < sidx[vr + 1]; s++) {
            out += std::to_string(q) + ' ' + strand + ' ' + std::to_string(seeds[s].start) + ' ' + std::to_string(seeds[s].len) + ' ' +
                   std::to_string(seeds[s].sa_end - seeds[s].sa_beg);
            for (uint64_t i = pidx[s]; i < pidx[s + 1]; i++) out += ' ' + std::to_string(pos[i]);
            out += '\n';
        }
        if (out.size() > (1u << 20)) {
            std::fwrite(out.data(), 1, out.size(), stdout);
            out.clear();
        }
    }
    std::fwrite(out.data(), 1, out.size(), stdout);
    std::fflush(stdout);
    std::fprintf(stderr, "[info] reads: %llu, seeds: %llu, located seeds: %llu, positions: %llu\n", (unsigned long long)Q,
                 (unsigned long long)rep.seeds, (unsigned long long)rep.located_seeds, (unsigned long long)rep.positions);
    return 0;
}

int fmindex_query_main(const Args &a)
{
    if (!a.seeds.empty()) { // (the text itself is not needed)
        Fmi f(a.sa_intv, 0);
        f.load(a.fasta + ".fmi");
        return seeds_main(a, f);
    }
    std::vector<uint8_t> S;
    {
        DeviceText T(a.fasta, a.device);
        S = T.to_host();
    }
    Fmi f(a.sa_intv, 0);
    f.load(a.fasta + ".fmi");
    if (!a.query.empty() && a.mismatches >= 0) {
        std::vector<uint8_t> q;
        for (unsigned char c : a.query) q.push_back(to_code(c));
        const MmHits h = mm_query(f, q.data(), (uint32_t)q.size(), 1, (uint32_t)a.mismatches, a.device);
        std::string qs, classes;
        for (auto c : q) qs.push_back("ACGT"[c]);
        for (int j = 0; j <= a.mismatches; j++)
            classes += (j ? ", " : "") + std::to_string(h.counts[j]) + (j == 0 ? " exact" : j == 1 ? " with 1 mismatch" : " with " + std::to_string(j) + " mismatches");
        std::fprintf(stderr, "[info] query = %s found %llu times (%s)\n", qs.c_str(), (unsigned long long)h.total, classes.c_str());
        for (size_t i = 0; i < std::min<size_t>(a.headn, h.total); i++) {
            std::string sub;
            for (size_t j = 0; j < q.size() && h.positions[i] + j < S.size(); j++) sub.push_back("ACGT"[S[h.positions[i] + j]]);
            std::fprintf(stderr, "[info] The %zu-%s position is %u, %u mismatches, content of substring is %s\n", i + 1,
                         ending(i + 1), h.positions[i], (unsigned)h.mismatches[i], sub.c_str());
        }
    } else if (!a.query.empty()) {
        std::vector<uint8_t> q;
        for (unsigned char c : a.query) q.push_back(to_code(c));
        uint32_t beg = 0, end = 0;
        uint64_t hits = 0, chk = 0;
        f.query(q.data(), (uint32_t)q.size(), 1, &beg, &end, &hits, &chk, nullptr, nullptr, 0, a.device);
        std::vector<uint32_t> off(hits + 1);
        std::vector<uint64_t> idx(2);
        if (hits)
            f.query(q.data(), (uint32_t)q.size(), 1, &beg, &end, &hits, &chk, off.data(), idx.data(), hits, a.device);
        std::string qs;
        for (auto c : q) qs.push_back("ACGT"[c]);
        std::fprintf(stderr, "[info] query = %s found %llu times\n", qs.c_str(), (unsigned long long)hits);
        for (size_t i = 0; i < std::min<size_t>(a.headn, hits); i++) {
            std::string sub;
            for (size_t j = 0; j < q.size() && off[i] + j < S.size(); j++) sub.push_back("ACGT"[S[off[i] + j]]);
            std::fprintf(stderr, "[info] The %zu-%s position is %u, content of substring is %s\n", i + 1, ending(i + 1), off[i],
                         sub.c_str());
        }
    }
    if (!a.batch.empty()) {
        std::ifstream p(a.batch, std::ios::binary);
        if (!p) throw std::runtime_error("cannot open " + a.batch);
        uint32_t L = 0, Q = 0;
        p.read(reinterpret_cast<char *>(&L), 4);
        p.read(reinterpret_cast<char *>(&Q), 4);
        std::fprintf(stderr, "[info] query_len: %u, num_query: %u\n", L, Q);
        std::vector<uint8_t> pat((size_t)L * Q);
        p.read(reinterpret_cast<char *>(pat.data()), (std::streamsize)pat.size());
        if (!p) throw std::runtime_error("truncated pattern file");
        for (auto &c : pat) c = to_code(c);
        std::vector<uint32_t> beg(Q), end(Q);
        uint64_t hits = 0, chk = 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (a.mismatches >= 0) {
            const MmHits h = mm_query(f, pat.data(), L, Q, (uint32_t)a.mismatches, a.device);
            hits = h.total;
            chk = h.rep.checksum;
            for (int j = 0; j <= a.mismatches; j++)
                std::fprintf(stderr, "[info] matched locations with %d mismatches: %llu\n", j, (unsigned long long)h.rep.hits[j]);
        } else {
            f.query(pat.data(), L, Q, beg.data(), end.data(), &hits, &chk, nullptr, nullptr, 0, a.device);
        }
        std::fprintf(stderr, "[info] searching time: %.6f seconds\n", seconds_since(t0));
        std::fprintf(stderr, "[info] number of matched locations: %llu\n", (unsigned long long)hits);
        std::fprintf(stderr, "[info] location checksum: %llu\n", (unsigned long long)chk);
    }
    return 0;
}

// ---- -g / --generic: texts over the byte alphabet ---------------------------------------------------------------------
bool given(const Args &a, const char *name) { return std::find(a.seen.begin(), a.seen.end(), name) != a.seen.end(); }

void check_generic_options(const Args &a)
{
    if (a.devices.size() > 1)
        throw std::runtime_error(std::string("--generic: one device only (not with ") + (given(a, "--devices") ? "--devices" : "--gpus") +
                                 " above 1)");
    for (const char *o : {"--lookup-len", "--exact", "--mismatches"})
        if (given(a, o)) throw std::runtime_error(std::string("--generic: ") + o + " is not supported for byte texts");
}

std::vector<uint8_t> read_bytes(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) throw std::runtime_error("cannot open " + path);
    in.seekg(0, std::ios::end);
    const std::streamoff size = in.tellg();
    in.seekg(0, std::ios::beg);
    std::vector<uint8_t> S((size_t)(size > 0 ? size : 0));
    if (!S.empty()) in.read(reinterpret_cast<char *>(S.data()), (std::streamsize)S.size());
    if (!in) throw std::runtime_error("cannot read " + path);
    return S;
}

void write_u32(const std::string &path, const std::vector<uint32_t> &v)
{
    std::ofstream o(path, std::ios::binary);
    if (!o) throw std::runtime_error("cannot write " + path);
    o.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(uint32_t)));
}

// printable ASCII as it is, every other byte (and the backslash) as \xHH
std::string escaped(const uint8_t *p, size_t len)
{
    std::string s;
    char buf[8];
    for (size_t i = 0; i < len; i++) {
        if (p[i] >= 0x20 && p[i] < 0x7F && p[i] != '\\') {
            s.push_back((char)p[i]);
        } else {
            std::snprintf(buf, sizeof buf, "\\x%02X", (unsigned)p[i]);
            s += buf;
        }
    }
    return s;
}

int generic_suffix_sort_main(const Args &a)
{
    const std::vector<uint8_t> S = read_bytes(a.fasta);
    if (given(a, "--kordered") || given(a, "--sorting-algorithm"))
        std::fprintf(stderr, "[info] --generic: -k and -s are ignored, the suffix array of a byte text is always exact\n");
    std::vector<uint32_t> SA(S.size() + 1), LCP;
    const auto t0 = std::chrono::steady_clock::now();
    check(kiss_hip_suffix_sort_u8(S.data(), S.size(), SA.data(), a.device), "kiss_hip_suffix_sort_u8");
    std::fprintf(stderr, "[info] n = %llu, k = %llu, suffix sorting elapsed %.6f\n", (unsigned long long)S.size(), ~0ull,
                 seconds_since(t0));
    if (!a.output_sa.empty()) write_u32(a.output_sa, SA);
    if (!a.output_lcp.empty()) {
        LCP.resize(S.size() + 1);
        const auto tl = std::chrono::steady_clock::now();
        check(kiss_hip_lcp_u8(S.data(), S.size(), SA.data(), nullptr, LCP.data(), a.device), "kiss_hip_lcp_u8");
        std::fprintf(stderr, "[info] LCP array elapsed %.6f\n", seconds_since(tl));
        write_u32(a.output_lcp, LCP);
    }
    return 0;
}

// FILE.fmi8: "KISSFMI8", u32 version, u32 sa_intv, u64 N, u32 pri, u32 sigma, then C, map, bwt, occ1, occ2, sa,
// b, b_occ, each as a u64 count of entries + little-endian entries (b / b_occ: count 0 when sa_intv == 1)
struct Fmi8 {
    static constexpr uint32_t FORMAT_VERSION = 1;
    kiss_hip_fmi8_sizes z{};
    uint32_t sa_intv = 4, pri = 0, sigma = 0;
    std::vector<uint32_t> C, occ1, sa, b_occ;
    std::vector<uint8_t> map, bwt;
    std::vector<uint16_t> occ2;
    std::vector<uint64_t> b;
    void alloc(uint64_t n)
    {
        check(kiss_hip_fmi8_sizes_for(n, sa_intv, sigma, &z), "kiss_hip_fmi8_sizes_for");
        C.assign(257, 0);
        map.assign(256, 0);
        bwt.assign(z.bwt_bytes, 0);
        occ1.assign(z.occ1_entries, 0);
        occ2.assign(z.occ2_entries, 0);
        sa.assign(z.sa_entries, 0);
        b.assign(z.b_words, 0);
        b_occ.assign(z.b_occ_entries, 0);
    }
    template <typename T> static void put(std::ofstream &o, const std::vector<T> &v)
    {
        const uint64_t count = v.size();
        o.write(reinterpret_cast<const char *>(&count), 8);
        o.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
    }
    template <typename T> static void get(std::ifstream &in, std::vector<T> &v, const char *name)
    {
        uint64_t count = 0;
        in.read(reinterpret_cast<char *>(&count), 8);
        if (!in) throw std::runtime_error("truncated .fmi8");
        if (count != v.size()) throw std::runtime_error(std::string("bad ") + name + " size in .fmi8");
        in.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
        if (!in) throw std::runtime_error("truncated .fmi8");
    }
    void save(const std::string &path) const
    {
        std::ofstream o(path, std::ios::binary);
        if (!o) throw std::runtime_error("cannot write " + path);
        const uint32_t version = FORMAT_VERSION;
        o.write("KISSFMI8", 8);
        o.write(reinterpret_cast<const char *>(&version), 4);
        o.write(reinterpret_cast<const char *>(&sa_intv), 4);
        o.write(reinterpret_cast<const char *>(&z.n_sa), 8);
        o.write(reinterpret_cast<const char *>(&pri), 4);
        o.write(reinterpret_cast<const char *>(&sigma), 4);
        put(o, C);
        put(o, map);
        put(o, bwt);
        put(o, occ1);
        put(o, occ2);
        put(o, sa);
        put(o, b);
        put(o, b_occ);
        if (!o) throw std::runtime_error("cannot write " + path);
    }
    void load(const std::string &path)
    {
        std::ifstream in(path, std::ios::binary);
        if (!in) throw std::runtime_error("cannot open " + path + " (run -g fmindex_build first)");
        char magic[8];
        uint32_t version = 0;
        uint64_t N = 0;
        in.read(magic, 8);
        if (!in) throw std::runtime_error("truncated .fmi8");
        if (std::memcmp(magic, "KISSFMI8", 8) != 0) throw std::runtime_error("not a .fmi8 file (bad magic)");
        in.read(reinterpret_cast<char *>(&version), 4);
        in.read(reinterpret_cast<char *>(&sa_intv), 4);
        in.read(reinterpret_cast<char *>(&N), 8);
        in.read(reinterpret_cast<char *>(&pri), 4);
        in.read(reinterpret_cast<char *>(&sigma), 4);
        if (!in) throw std::runtime_error("truncated .fmi8");
        if (version != FORMAT_VERSION) throw std::runtime_error(".fmi8 format version " + std::to_string(version) + " is not supported");
        if (N == 0 || pri >= N || sigma > 256 || sa_intv < 1 || sa_intv > KISS_HIP_FMI_MAX_SA_INTV) throw std::runtime_error("bad .fmi8 header");
        alloc(N - 1);
        get(in, C, "C");
        get(in, map, "map");
        get(in, bwt, "bwt");
        get(in, occ1, "occ1");
        get(in, occ2, "occ2");
        get(in, sa, "sa");
        get(in, b, "b");
        get(in, b_occ, "b_occ");
        if (in.peek() != EOF) throw std::runtime_error("trailing bytes in .fmi8");
    }
    kiss_hip_fmi8_view view() const
    {
        kiss_hip_fmi8_view v{};
        v.n_sa = z.n_sa;
        v.pri = pri;
        v.sa_intv = sa_intv;
        v.sigma = sigma;
        v.C = C.data();
        v.map = map.data();
        v.bwt = bwt.data();
        v.occ1 = occ1.data();
        v.occ2 = occ2.data();
        v.sa = sa.data();
        v.b = sa_intv == 1 ? nullptr : b.data();
        v.b_occ = sa_intv == 1 ? nullptr : b_occ.data();
        return v;
    }
};

int generic_fmindex_build_main(const Args &a)
{
    const std::vector<uint8_t> S = read_bytes(a.fasta);
    if (given(a, "--kordered")) std::fprintf(stderr, "[info] --generic: -k is ignored, the index is built from the exact suffix array\n");
    Fmi8 f;
    f.sa_intv = a.sa_intv;
    // the census first: the arrays are sized by the number of distinct byte values
    check(kiss_hip_fmi8_build_host(S.data(), S.size(), nullptr, f.sa_intv, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, &f.sigma, &f.pri, a.device),
          "kiss_hip_fmi8_build_host");
    f.alloc(S.size());
    check(kiss_hip_fmi8_build_host(S.data(), S.size(), nullptr, f.sa_intv, f.sigma, f.C.data(), f.map.data(), f.bwt.data(),
                                   f.occ1.data(), f.occ2.data(), f.sa.data(), f.b.data(), f.b_occ.data(), &f.sigma, &f.pri, a.device),
          "kiss_hip_fmi8_build_host");
    f.save(a.fasta + ".fmi8");
    return 0;
}

int generic_fmindex_query_main(const Args &a)
{
    const std::vector<uint8_t> S = read_bytes(a.fasta);
    Fmi8 f;
    f.load(a.fasta + ".fmi8");
    const kiss_hip_fmi8_view v = f.view();
    // counts first (they size the output), then the positions of every pattern in ascending order
    auto run = [&](const uint8_t *pat, const std::vector<uint64_t> &pidx, std::vector<uint32_t> &pos, std::vector<uint64_t> &idx,
                   uint64_t &hits, uint64_t &chk) {
        const uint64_t Q = pidx.size() - 1;
        std::vector<uint32_t> beg(Q + 1), end(Q + 1);
        check(kiss_hip_fmi8_query_host(&v, pat, pidx.data(), Q, beg.data(), end.data(), &hits, &chk, nullptr, nullptr, 0, nullptr,
                                       a.device),
              "kiss_hip_fmi8_query_host");
        pos.assign(hits + 1, 0);
        idx.assign(Q + 1, 0);
        check(kiss_hip_fmi8_query_host(&v, pat, pidx.data(), Q, beg.data(), end.data(), &hits, &chk, pos.data(), idx.data(), hits,
                                       nullptr, a.device),
              "kiss_hip_fmi8_query_host");
    };
    if (!a.query.empty()) {
        const uint8_t *q = reinterpret_cast<const uint8_t *>(a.query.data());
        std::vector<uint32_t> pos;
        std::vector<uint64_t> idx;
        uint64_t hits = 0, chk = 0;
        run(q, {0, a.query.size()}, pos, idx, hits, chk);
        std::fprintf(stderr, "[info] query = %s found %llu times\n", escaped(q, a.query.size()).c_str(), (unsigned long long)hits);
        for (size_t i = 0; i < std::min<size_t>(a.headn, hits); i++) {
            const size_t len = std::min<size_t>(a.query.size(), S.size() - std::min<size_t>(S.size(), pos[i]));
            std::fprintf(stderr, "[info] The %zu-%s position is %u, content of substring is %s\n", i + 1, ending(i + 1), pos[i],
                         escaped(S.data() + pos[i], len).c_str());
        }
    }
    if (!a.batch.empty()) {
        std::ifstream p(a.batch, std::ios::binary);
        if (!p) throw std::runtime_error("cannot open " + a.batch);
        uint32_t L = 0, Q = 0;
        p.read(reinterpret_cast<char *>(&L), 4);
        p.read(reinterpret_cast<char *>(&Q), 4);
        std::fprintf(stderr, "[info] query_len: %u, num_query: %u\n", L, Q);
        if (!p || (L == 0 && Q != 0)) throw std::runtime_error("bad pattern file");
        std::vector<uint8_t> pat((size_t)L * Q);
        p.read(reinterpret_cast<char *>(pat.data()), (std::streamsize)pat.size());
        if (!p) throw std::runtime_error("truncated pattern file");
        std::vector<uint64_t> pidx((size_t)Q + 1);
        for (uint64_t q = 0; q <= Q; q++) pidx[q] = q * L;
        std::vector<uint32_t> pos;
        std::vector<uint64_t> idx;
        uint64_t hits = 0, chk = 0;
        const auto t0 = std::chrono::steady_clock::now();
        run(pat.data(), pidx, pos, idx, hits, chk);
        std::fprintf(stderr, "[info] searching time: %.6f seconds\n", seconds_since(t0));
        std::fprintf(stderr, "[info] number of matched locations: %llu\n", (unsigned long long)hits);
        std::fprintf(stderr, "[info] location checksum: %llu\n", (unsigned long long)chk);
    }
    return 0;
}

} // namespace

int main(int argc, char **argv)
{
    try {
        Args a = parse(argc, argv);
        if (a.generic) { // the reference's TODO (suffix_sort.hpp:26-28): texts over the byte alphabet
            check_generic_options(a);
            if (a.command == "suffix_sort") return generic_suffix_sort_main(a);
            if (a.command == "fmindex_build") return generic_fmindex_build_main(a);
            if (a.command == "fmindex_query") return generic_fmindex_query_main(a);
            usage();
            throw std::runtime_error("invalid command '" + a.command + "'");
        }
        if (a.command == "suffix_sort") return suffix_sort_main(a);
        if (a.command == "fmindex_build") return fmindex_build_main(a);
        if (a.command == "fmindex_query") return fmindex_query_main(a);
        usage();
        throw std::runtime_error("invalid command '" + a.command + "'");
    } catch (const std::exception &e) {
        std::cerr << e.what() << std::endl;
        return 1;
    }
}
