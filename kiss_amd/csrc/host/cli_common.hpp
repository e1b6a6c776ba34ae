// cli_common.hpp -- what the sub-commands of `kiss` share: the version, usage(), the options (Args, one table, parse()),
// check() and the text loaded through the device parser (DeviceText).  Part of the one translation unit kiss_cli.cpp.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include "cli_bam_index.hpp"
#include "../../../include/kiss_hip.h"
#include "../../../include/kiss_hip_insert.h"
#include "../../../include/kiss_hip_pileup.h"

namespace kiss_cli {

inline const char *const VERSION = "1.0.0-hip";

inline void usage()
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

// The help of the read files (`kiss --help-reads`).  Kept apart from usage(): what `kiss -h` prints is recorded byte for byte
// (tests/golden/cli_parse_recording.json) and stays as it is.
inline void usage_reads()
{
    std::cerr << "The read files of ./kiss fmindex_query --seeds READS [--mates READS2]:\n"
              << "  --reads-format FORMAT (=auto)  auto: FASTQ if the first byte of the file is '@', otherwise lines;\n"
              << "                                 lines: one read per line, ACGT, any other letter is no base; empty lines and\n"
              << "                                 lines that start with '>' are no reads, the word behind '>' on the line\n"
              << "                                 directly in front of a read is its name (else its number);\n"
              << "                                 fastq: records of four lines: @name, the bases, +, the qualities (as many as\n"
              << "                                 bases); anything else is refused with the number of the first bad record\n"
              << "                                 (no multi-line FASTQ, no gzip).  With --sam the QUAL column of a FASTQ read is\n"
              << "                                 its quality string, reversed where SEQ is; of a read from lines it is *.\n"
              << "                                 With --mates both files have one format, and a FASTQ name that ends in /1 or\n"
              << "                                 /2 loses those two bytes.  A FASTQ read without bases stops the command.\n"
              << "                                 The files are parsed on the device (line ends may be \\n or \\r\\n).\n"
              << "  --batch-reads NUM (=0)         with --sam: the file is mapped NUM reads (with --mates: NUM pairs) at a time, so a file\n"
              << "                                 of any size goes through; 0: the whole file as one batch.  The SAM does not depend\n"
              << "                                 on NUM: record, read and pair numbers in messages and the QNAMEs of reads without a\n"
              << "                                 name count through the file.  The header is written once.  An error found in a\n"
              << "                                 later batch (a bad FASTQ record, a read without bases, a mate file that runs out)\n"
              << "                                 comes behind the SAM lines of the batches before it, with a non-zero exit status.\n"
              << "                                 With --ins-auto the insert size is estimated once, from the first batch, and its\n"
              << "                                 [insert] line is printed once; those values serve every later batch.\n"
              << "  --batch-chunk BYTES (=67108864)  with --batch-reads: the file is read BYTES at a time, and on (twice as much each\n"
              << "                                 time) until NUM records or the file's end are in memory; the records are cut on\n"
              << "                                 the device.\n";
}

// The help of the SAM tags that are asked for (`kiss --help-sam`): apart from usage() for the same reason.
inline void usage_sam()
{
    std::cerr << "The optional SAM tags of ./kiss fmindex_query --seeds READS --chain --align --sam:\n"
              << "  --md                           with --sam: every mapped line carries MD:Z:, directly behind NM:i: -- the text\n"
              << "                                 under the alignment for a reader without the genome: numbers of matching\n"
              << "                                 columns, the text's letter at a mismatch (a read letter that is no base never\n"
              << "                                 matches), ^ and the text's letters at a deletion; an insertion does not end a\n"
              << "                                 run of matches.  The strings are written on the device.  Unmapped lines carry\n"
              << "                                 none.  Without --md every byte of the output is what it was.\n"
              << "Who writes the alignment lines:\n"
              << "  --sam-writer host|device (=host)\n"
              << "                                 with --sam: host builds every line on one thread of the host, from the arrays the\n"
              << "                                 stages left behind; device writes the same bytes on the device\n"
              << "                                 (kiss_hip_fmi_sam_host) and prints them batch by batch.  The header is the host's\n"
              << "                                 in both.  A pair that is bad input ends the run with the same message and a\n"
              << "                                 non-zero status under both writers; the host writer prints the lines of the pairs in\n"
              << "                                 front of it first, the device writer the lines of the EARLIER BATCHES only: the\n"
              << "                                 device call writes nothing for a batch that has a bad read.\n";
}

// The help of the options of --mates that `kiss -h` does not list (`kiss --help-pairs`): apart from usage() for the same reason.
inline void usage_pairs()
{
    std::cerr << "The insert size of ./kiss fmindex_query --seeds READS --mates READS2 --chain --align --sam:\n"
              << "  --ins-auto                     with --mates: --ins-min, --ins-max and --ins-mean are estimated from the reads, on the\n"
              << "                                 device, before the mates are paired (and before --rescue lays its windows): from\n"
              << "                                 the pairs whose first mappings lie on one record, face each other in order and\n"
              << "                                 have a MAPQ of --ins-auto-min-mapq or more, the quartiles of the insert, then mean\n"
              << "                                 and deviation without the outliers (more than 2 interquartile ranges outside the\n"
              << "                                 quartiles); --ins-min = min(q25 - 3 IQR, mean - 4 sd), not below 0, --ins-max =\n"
              << "                                 max(q75 + 3 IQR, mean + 4 sd), --ins-mean = mean.  With fewer than\n"
              << "                                 --ins-auto-min-pairs such pairs the values given (or their defaults) are used.\n"
              << "                                 One line on stderr says what was found:\n"
              << "                                 [insert] pairs= samples= used= q25= q50= q75= mean= sd= ins_min= ins_max= applied=\n"
              << "                                 Forward-then-reverse libraries only.  Without --ins-auto every byte of the output\n"
              << "                                 is what it was.\n"
              << "  --ins-auto-min-mapq NUM (=20)  lowest MAPQ of either mate of a pair that is looked at\n"
              << "  --ins-auto-max NUM (=10000)    longest insert that is looked at (1..65535)\n"
              << "  --ins-auto-min-pairs NUM (=25) fewest such pairs for an estimate\n";
}

// The help of the pileup file (`kiss --help-pileup`): apart from usage() for the same reason.
inline void usage_pileup()
{
    std::cerr << "The pileup of ./kiss fmindex_query --seeds READS [--mates READS2] --chain --align --sam:\n"
              << "  --pileup FILE                  with --sam: what the mappings say at every position of the text, counted on the\n"
              << "                                 device and summed over the batches of --batch-reads in one array of 32 bytes per\n"
              << "                                 base of the text, which is allocated before a read is mapped.  FILE gets one line\n"
              << "                                 per position that a read covers, deletes or inserts behind, tab-separated:\n"
              << "                                 RNAME POS REF COV A C G T N DEL INS -- the record and the 1-based position in it,\n"
              << "                                 the text's letter, the aligned read bases over it, those bases by letter (N: no\n"
              << "                                 base), the reads that delete the position, the insertions directly behind it.\n"
              << "                                 The depth in samtools' sense is COV + DEL.  Counted are the primary and the\n"
              << "                                 supplementary lines of a read; with --mates the one line of either mate that the\n"
              << "                                 pair chose, with the pair's MAPQ.  Mates that overlap are counted twice.  The SAM\n"
              << "                                 on stdout is what it is without the option.\n"
              << "  --pileup-min-mapq NUM (=0)     lowest MAPQ of a line that is counted (0..255)\n"
              << "  --pileup-proper                with --mates: only the mates of proper pairs are counted\n";
}

// The help of the BAM output (`kiss --help-bam`): apart from usage() for the same reason.
inline void usage_bam()
{
    std::cerr << "BAM in the place of SAM, ./kiss fmindex_query --seeds READS [--mates READS2] --chain --align --sam --bam FILE:\n"
              << "  --bam FILE                     with --sam: the mappings go to FILE as BAM ('-': stdout) and no SAM line is\n"
              << "                                 printed.  One SAM line is one BAM record: the same reads, flags, places and\n"
              << "                                 tags (NM, MD with --md, AS, XS, YS, YT, YR), the tag values as unsigned 32-bit\n"
              << "                                 integers.  The records and the BGZF blocks around them, with the CRC-32 of every\n"
              << "                                 block, are written on the device (kiss_hip_fmi_bam_host, kiss_hip_bgzf_host).\n"
              << "                                 The blocks are NOT compressed (stored deflate blocks), which every BAM reader\n"
              << "                                 accepts: `samtools sort` writes the compressed file.  Works with --mates,\n"
              << "                                 --rescue, --md, --ins-auto, --batch-reads and --pileup.  A read name of more than\n"
              << "                                 254 bytes, more than 65535 CIGAR operations on a line or a position of 2^31 or\n"
              << "                                 more in its record cannot be written as BAM and ends the run.  Without --bam every\n"
              << "                                 byte of the output is what it was.\n"
              << "  --bam-compress                 with --bam: the header, every batch and the end-of-file block go out in COMPRESSED\n"
              << "                                 BGZF blocks: DEFLATE (LZ77 matches, fixed or dynamic Huffman codes, whichever is\n"
              << "                                 smallest for the block; a block that does not shrink stays stored), computed on the\n"
              << "                                 device, one block per workgroup (kiss_hip_bgzf_deflate_host).  The file decompresses\n"
              << "                                 to exactly what --bam alone writes and is smaller; no `samtools` pass is needed.\n"
              << "  --bam-sort                     with --bam: the records of the WHOLE file in coordinate order (reference, then\n"
              << "                                 position; records without a place last; equal places in the order of the reads),\n"
              << "                                 sorted on the device (kiss_hip_bam_sort_host), and SO:coordinate in the @HD line:\n"
              << "                                 `samtools index` takes the file as it is and no `samtools sort` pass is needed.\n"
              << "                                 The unframed records of every batch are kept in host memory until the last one,\n"
              << "                                 then sorted once, framed and written: nothing reaches FILE before that.  Works\n"
              << "                                 with --batch-reads, --bam-compress and --bam -.\n"
              << "  --bam-index                    with --bam FILE --bam-sort: FILE.bai, the BAI index of the sorted file, built on the\n"
              << "                                 device (kiss_hip_bai_host) from the sorted records and the offsets of their blocks\n"
              << "                                 and written behind FILE: region queries (`samtools view FILE chr:beg-end`, IGV)\n"
              << "                                 need no `samtools index` pass.  One chunk per run of records that share a bin: a\n"
              << "                                 valid index per the specification, not byte for byte the one `samtools index`\n"
              << "                                 writes.  References or alignments beyond 2^29 are refused: the CSI index is not\n"
              << "                                 built, and since the index is complete in memory before the first byte of FILE is\n"
              << "                                 written, such a run ends with FILE empty.  Not with --bam -: an index of what goes\n"
              << "                                 to stdout has no name.\n"
              << "  --bam-markdup                  with --bam FILE --bam-sort: the duplicate templates of the WHOLE file get FLAG 0x400\n"
              << "                                 on the device (kiss_hip_bam_markdup_host), directly before the sort, while the\n"
              << "                                 records of a read are still together: no `samtools fixmate` / `samtools markdup`\n"
              << "                                 or Picard pass is needed.  A template is the records of one read name; its ends\n"
              << "                                 are the unclipped 5' ends of its mapped primary records with their strands.  Of\n"
              << "                                 the pairs with the same two ends the one with the highest sum of base qualities\n"
              << "                                 stays unmarked (ties: the first in the file); a single mapped read is marked when\n"
              << "                                 a pair has its end, else all but the best of an end.  Every record of a marked\n"
              << "                                 template is marked, secondary, supplementary and an unmapped mate included.  Only\n"
              << "                                 the FLAG of records changes, no size and no place: stdout is what it is without\n"
              << "                                 the option, and so is FILE.bai (with --bam-compress as long as the compressed\n"
              << "                                 blocks keep their sizes: a block that packs differently moves those behind it).\n"
              << "                                 One line of counts goes to stderr.\n"
              << "  --bam-markdup-min-qual Q       with --bam-markdup: a base quality counts towards the sum from Q (15, Picard's\n"
              << "                                 SUM_OF_BASE_QUALITIES; 0: every quality).\n";
}

inline void check(int rc, const char *where)
{
    if (rc != KISS_HIP_OK) throw std::runtime_error(std::string(where) + ": " + kiss_hip_strerror(rc));
}

inline double seconds_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
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
        create_s = seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        const int rc = kiss_hip_ctx_load_text_file(ctx, path.c_str(), &d_S, &n);
        load_s = seconds_since(t0);
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
    std::string reads_format = "auto"; // --reads-format auto | lines | fastq
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
    bool md = false;     // fmindex_query ... --sam --md
    kiss_hip_rescue_params rescue_params{0, 1000, 4, 0, 960}; // (ins_min / ins_max: the pair parameters' that are used, set in map_reads)
    bool ins_auto = false; // fmindex_query ... --mates READS2 --sam --ins-auto
    kiss_hip_insert_params insert_params{20, 10000, 25, 2, 3, 4};
    size_t batch_reads = 0;          // fmindex_query ... --sam --batch-reads N (0: the whole file as one batch)
    size_t batch_chunk = 64u << 20;  // --batch-chunk BYTES
    std::string sam_writer = "host"; // fmindex_query ... --sam --sam-writer host|device
    std::string pileup;              // fmindex_query ... --sam --pileup FILE
    kiss_hip_pileup_params pileup_params{0, KISS_HIP_HIT_SECONDARY, 0, 0};
    bool pileup_proper = false;      // --pileup-proper
    std::string bam;                 // fmindex_query ... --sam --bam FILE ('-': stdout)
    bool bam_compress = false;       // --bam-compress: the BGZF blocks compressed on the device
    bool bam_sort = false;           // --bam-sort: the records of the whole file in coordinate order, sorted on the device
    bool bam_index = false;          // --bam-index: FILE.bai beside the sorted FILE, built on the device
    bool bam_markdup = false;        // --bam-markdup: FLAG 0x400 on the duplicate templates of the whole file, marked on the device
    uint32_t bam_markdup_min_qual = 15; // --bam-markdup-min-qual Q
};

inline bool given(const Args &a, const char *name) { return std::find(a.seen.begin(), a.seen.end(), name) != a.seen.end(); }

// One row per option: its long name, its short one, the member it sets (a bool takes no value; nothing: the value is read and
// dropped), whether it is recorded in Args::seen, and the options it goes with, asked for in that order.  parse() asks the
// "X goes with Y" rules in row order, so a command line that breaks two of them gets the message of the earlier row.
typedef std::variant<std::monostate, bool *, uint32_t *, int *, long long *, size_t *, std::string *, std::vector<int> *> Target;
struct Opt {
    const char *name, *alias;
    Target (*at)(Args &);
    bool seen = false;
    const char *with[2] = {nullptr, nullptr};
};
#define KISS_AT(member) [](Args &a) -> Target { return &a.member; }
inline const Opt OPTIONS[] = {
    {"--generic", "-g", KISS_AT(generic)},
    {"--verbose", nullptr, KISS_AT(verbose)},
    {"--num_threads", "-t", [](Args &) -> Target { return {}; }},
    {"--device", nullptr, KISS_AT(device)},
    {"--kordered", "-k", KISS_AT(k), true},
    {"--sorting-algorithm", "-s", KISS_AT(algo), true},
    {"--query", "-q", KISS_AT(query)},
    {"--headn", "-n", KISS_AT(headn)},
    {"--batch", "-b", KISS_AT(batch)},
    {"--output-sa", nullptr, KISS_AT(output_sa)},
    {"--output-lcp", nullptr, KISS_AT(output_lcp)},
    {"--sa-intv", nullptr, KISS_AT(sa_intv), true},
    {"--lookup-len", nullptr, KISS_AT(lookup_len), true},
    {"--gpus", nullptr, KISS_AT(gpus), true},
    {"--devices", nullptr, KISS_AT(devices), true},
    {"--exact", nullptr, KISS_AT(exact), true},
    {"--mismatches", nullptr, KISS_AT(mismatches), true},
    {"--seeds", nullptr, KISS_AT(seeds), true},
    {"--min-seed-len", nullptr, KISS_AT(min_seed_len), true, {"--seeds"}},
    {"--max-seed-len", nullptr, KISS_AT(max_seed_len), true, {"--seeds"}},
    {"--max-occ", nullptr, KISS_AT(max_occ), true, {"--seeds"}},
    {"--both-strands", nullptr, KISS_AT(both_strands), true, {"--seeds"}},
    {"--reads-format", nullptr, KISS_AT(reads_format), true, {"--seeds"}},
    {"--max-gap", nullptr, KISS_AT(chain_params.max_gap), true, {"--chain"}},
    {"--band", nullptr, KISS_AT(chain_params.band), true, {"--chain"}},
    {"--gap-cost", nullptr, KISS_AT(chain_params.gap_cost), true, {"--chain"}},
    {"--max-lookback", nullptr, KISS_AT(chain_params.max_lookback), true, {"--chain"}},
    {"--min-chain-score", nullptr, KISS_AT(chain_params.min_score), true, {"--chain"}},
    {"--align", nullptr, KISS_AT(align), true, {"--chain"}},
    {"--match", nullptr, KISS_AT(align_params.match), true, {"--chain", "--align"}},
    {"--mismatch", nullptr, KISS_AT(align_params.mismatch), true, {"--chain", "--align"}},
    {"--gap-open", nullptr, KISS_AT(align_params.gap_open), true, {"--chain", "--align"}},
    {"--gap-extend", nullptr, KISS_AT(align_params.gap_extend), true, {"--chain", "--align"}},
    {"--align-band", nullptr, KISS_AT(align_params.band), true, {"--chain", "--align"}},
    {"--chain", nullptr, KISS_AT(chain), true, {"--seeds"}},
    {"--sam", nullptr, KISS_AT(sam), true, {"--align"}},
    {"--min-map-score", nullptr, KISS_AT(select_params.min_score), true, {"--sam"}},
    {"--overlap", nullptr, KISS_AT(select_params.overlap), true, {"--sam"}},
    {"--mapq-coef", nullptr, KISS_AT(select_params.mapq_coef), true, {"--sam"}},
    {"--mapq-max", nullptr, KISS_AT(select_params.mapq_max), true, {"--sam"}},
    {"--max-hits", nullptr, KISS_AT(select_params.max_hits), true, {"--sam"}},
    {"--mates", nullptr, KISS_AT(mates), true, {"--sam"}},
    {"--ins-min", nullptr, KISS_AT(pair_params.ins_min), true, {"--mates"}},
    {"--ins-max", nullptr, KISS_AT(pair_params.ins_max), true, {"--mates"}},
    {"--ins-mean", nullptr, KISS_AT(pair_params.ins_mean), true, {"--mates"}},
    {"--pair-pen-coef", nullptr, KISS_AT(pair_params.pen_coef), true, {"--mates"}},
    {"--pair-pen-max", nullptr, KISS_AT(pair_params.pen_max), true, {"--mates"}},
    {"--rescue", nullptr, KISS_AT(rescue), true, {"--mates"}},
    {"--rescue-anchors", nullptr, KISS_AT(rescue_params.max_anchors), true, {"--rescue"}},
    {"--rescue-min-anchor-score", nullptr, KISS_AT(rescue_params.min_anchor_score), true, {"--rescue"}},
    {"--rescue-width", nullptr, KISS_AT(rescue_params.max_width), true, {"--rescue"}},
    {"--md", nullptr, KISS_AT(md), true, {"--sam"}},
    {"--ins-auto", nullptr, KISS_AT(ins_auto), true, {"--mates"}},
    {"--ins-auto-min-mapq", nullptr, KISS_AT(insert_params.min_mapq), true, {"--ins-auto"}},
    {"--ins-auto-max", nullptr, KISS_AT(insert_params.max_insert), true, {"--ins-auto"}},
    {"--ins-auto-min-pairs", nullptr, KISS_AT(insert_params.min_samples), true, {"--ins-auto"}},
    {"--batch-reads", nullptr, KISS_AT(batch_reads), true, {"--sam"}},
    {"--batch-chunk", nullptr, KISS_AT(batch_chunk), true, {"--batch-reads"}},
    {"--sam-writer", nullptr, KISS_AT(sam_writer), true, {"--sam"}},
    {"--pileup", nullptr, KISS_AT(pileup), true, {"--sam"}},
    {"--pileup-min-mapq", nullptr, KISS_AT(pileup_params.min_mapq), true, {"--pileup"}},
    {"--pileup-proper", nullptr, KISS_AT(pileup_proper), true, {"--pileup", "--mates"}},
    {"--bam", nullptr, KISS_AT(bam), true, {"--sam"}},
    {"--bam-compress", nullptr, KISS_AT(bam_compress), true, {"--bam"}},
    {"--bam-sort", nullptr, KISS_AT(bam_sort), true, {"--bam"}},
    {"--bam-index", nullptr, KISS_AT(bam_index), true, {"--bam-sort"}},
    {"--bam-markdup", nullptr, KISS_AT(bam_markdup), true, {"--bam-sort"}},
    {"--bam-markdup-min-qual", nullptr, KISS_AT(bam_markdup_min_qual), true, {"--bam-markdup"}},
};
#undef KISS_AT

inline Args parse(int argc, char **argv)
{
    Args a;
    std::vector<std::string> pos;
    for (int i = 1; i < argc; i++) {
        const std::string s = argv[i];
        if (s == "-h" || s == "--help") { usage(); std::exit(1); }
        if (s == "-v" || s == "--version") { std::cerr << VERSION << std::endl; std::exit(1); }
        if (s == "--help-reads") { usage_reads(); std::exit(1); }
        if (s == "--help-sam") { usage_sam(); std::exit(1); }
        if (s == "--help-pairs") { usage_pairs(); std::exit(1); }
        if (s == "--help-pileup") { usage_pileup(); std::exit(1); }
        if (s == "--help-bam") { usage_bam(); std::exit(1); }
        const Opt *o = std::find_if(std::begin(OPTIONS), std::end(OPTIONS), [&](const Opt &x) { return s == x.name || (x.alias && s == x.alias); });
        if (o == std::end(OPTIONS)) {
            if (!s.empty() && s[0] == '-' && s.size() > 1) throw std::runtime_error("unrecognised option '" + s + "'");
            pos.push_back(s);
            continue;
        }
        if (o->seen) a.seen.push_back(o->name);
        const Target to = o->at(a);
        if (bool *const *flag = std::get_if<bool *>(&to)) { **flag = true; continue; }
        if (i + 1 >= argc) throw std::runtime_error(std::string("the required argument for option '") + o->name + "' is missing");
        const std::string v = argv[++i];
        if (auto p = std::get_if<uint32_t *>(&to)) **p = (uint32_t)std::stoul(v);
        else if (auto p = std::get_if<int *>(&to)) **p = std::stoi(v);
        else if (auto p = std::get_if<long long *>(&to)) **p = std::stoll(v);
        else if (auto p = std::get_if<size_t *>(&to)) **p = (size_t)std::stoull(v);
        else if (auto p = std::get_if<std::string *>(&to)) **p = v;
        else if (auto list = std::get_if<std::vector<int> *>(&to)) // --devices: comma-separated
            for (size_t at = 0; at <= v.size();) {
                const size_t comma = v.find(',', at);
                const std::string item = v.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
                if (item.empty()) throw std::runtime_error("--devices: empty entry in '" + v + "'");
                (*list)->push_back(std::stoi(item));
                if (comma == std::string::npos) break;
                at = comma + 1;
            }
    }
    if (pos.empty()) { usage(); std::exit(1); }
    if (a.gpus < 1) throw std::runtime_error("--gpus must be >= 1");
    if (a.sa_intv < 1 || a.sa_intv > KISS_HIP_FMI_MAX_SA_INTV) throw std::runtime_error("--sa-intv must be in 1..32");
    if (a.lookup_len > KISS_HIP_FMI_MAX_LOOKUP_LEN) throw std::runtime_error("--lookup-len must be in 0..14");
    if (a.mismatches < -1 || a.mismatches > (int)KISS_HIP_FMI_MAX_MISMATCHES) throw std::runtime_error("--mismatches must be in 0..3");
    const Opt *row = OPTIONS;
    const auto goes_with_through = [&](const char *last) { // the rules of the rows not yet asked, up to the row `last`
        do {
            for (const char *w : row->with)
                if (w && given(a, row->name) && !given(a, w)) throw std::runtime_error(std::string(row->name) + " goes with " + w);
        } while (std::strcmp((row++)->name, last));
    };
    goes_with_through("--max-hits");
    if (a.select_params.overlap > 256u || a.select_params.mapq_coef > 65535u || a.select_params.mapq_max > 255u)
        throw std::runtime_error("--overlap is at most 256, --mapq-coef at most 65535, --mapq-max at most 255");
    goes_with_through("--pair-pen-max");
    if (a.pair_params.ins_min > a.pair_params.ins_max || a.pair_params.pen_coef > 65535u || a.pair_params.pen_max > 65535u)
        throw std::runtime_error("--ins-min is at most --ins-max, --pair-pen-coef and --pair-pen-max at most 65535");
    goes_with_through("--rescue-width");
    if (a.rescue_params.max_anchors < 1 || a.rescue_params.max_width < 1 || a.rescue_params.max_width > KISS_HIP_ALIGN_MAX_BAND)
        throw std::runtime_error("--rescue-anchors is at least 1, --rescue-width in 1..1024");
    goes_with_through("--md");
    goes_with_through("--ins-auto-min-pairs");
    if (a.insert_params.max_insert < 1 || a.insert_params.max_insert > KISS_HIP_INSERT_MAX)
        throw std::runtime_error("--ins-auto-max is in 1..65535");
    goes_with_through("--batch-chunk");
    if (a.batch_chunk < 1 || a.batch_chunk > (1ull << 30)) throw std::runtime_error("--batch-chunk is in 1..1073741824");
    goes_with_through("--sam-writer");
    if (a.sam_writer != "host" && a.sam_writer != "device") throw std::runtime_error("--sam-writer is one of host, device (kiss --help-sam)");
    goes_with_through("--pileup-proper");
    if (a.pileup_params.min_mapq > 255u) throw std::runtime_error("--pileup-min-mapq is at most 255 (kiss --help-pileup)");
    a.pileup_params.proper_only = a.pileup_proper ? 1u : 0u;
    goes_with_through("--bam");
    if (given(a, "--bam") && a.bam.empty()) throw std::runtime_error("--bam needs a file name, or - for stdout (kiss --help-bam)");
    goes_with_through("--bam-index");
    bam_index_options(a.bam_index, a.bam);
    goes_with_through("--bam-markdup-min-qual");
    if (given(a, "--mates")) { // the pair's MAPQ is on the scale of the reads'; the mates face each other
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
    if (given(a, "--seeds")) {
        if (a.generic) throw std::runtime_error("--seeds is not supported for byte texts (--generic)");
        if (!a.query.empty() || !a.batch.empty() || a.mismatches >= 0)
            throw std::runtime_error("--seeds cannot be combined with -q, -b or --mismatches");
        if (a.min_seed_len < 1) throw std::runtime_error("--min-seed-len must be at least 1");
        if (a.reads_format != "auto" && a.reads_format != "lines" && a.reads_format != "fastq")
            throw std::runtime_error("--reads-format is one of auto, lines, fastq (kiss --help-reads)");
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

} // namespace kiss_cli
