// kiss_cli.cpp -- `kiss`: the kISS command line on top of libkiss_hip.so (host C++17, no HIP, no Boost).
//
// Keeps the reference's CLI surface (reference include/utils/options.hpp:83-203, src/main.cpp:19-39) and its log fields:
//   kiss [-h] [-v] [-g] [-t NUM] [--verbose] <command> [options] <FASTA filename/Text filename>
// usage() (cli_common.hpp) has every option.  The commands, and the library call behind each:
//   * suffix_sort (command/suffix_sort.hpp): kiss_hip_ctx_suffix_sort_dna_u32_dev; with --gpus N / --devices LIST sharded over
//     several GPUs by one process: kiss_hip_multi_suffix_sort_dna_u32_dev.  Extras: --output-sa FILE (raw u32 LE, n + 1 entries;
//     the reference never writes the SA), --output-lcp FILE (of an exact order: kiss_hip_ctx_lcp_dna_u32_dev, same format).
//   * fmindex_build (command/fmindex_build.hpp) -> <fasta>.fmi: kiss_hip_fmi_build_host; with --sa-intv N / --lookup-len L
//     (FMIndex<N>{.LOOKUP_LEN = L}; 4 and 0 are the reference CLI's) kiss_hip_fmi_build_ex_host; --exact: from the exact suffix
//     array (kiss_hip_suffix_sort_dna_u32), which the positions of --mismatches and --seeds need.
//   * fmindex_query -q STR [-n NUM] / -b patterns.bin (command/fmindex_query.hpp): kiss_hip_fmi_query_batch_host, or
//     kiss_hip_fmi_query_ex_host (the file records L, not N: --sa-intv N); with --mismatches E (0..3) every position within
//     Hamming distance E, ascending, each with its mismatch count: kiss_hip_fmi_query_mm_host.
//   * fmindex_query --seeds READS: the read-mapping pipeline (cli_reads.hpp; what it prints: cli_format.hpp), a stage per option:
//       the seeds of every read                       kiss_hip_fmi_seeds_host   -> read strand start len count pos...
//       --chain   chained into candidate loci         kiss_hip_fmi_chain_host   -> read strand score anchors rbeg rend tbeg tend
//       --align   every chain aligned to the text     kiss_hip_fmi_align_host   -> read strand score rbeg rend tbeg tend nm cigar
//       --sam     the mappings of a read picked       kiss_hip_fmi_select_host  -> SAM
//       --mates READS2   the mappings of two mates paired   kiss_hip_fmi_pair_host  -> paired SAM
//       --rescue  before that, the missing mate sought near its partner: kiss_hip_fmi_pair_host, kiss_hip_fmi_rescue_host, the
//                 align call, kiss_hip_fmi_aln_merge_host, the select call again
//       --ins-auto  before the pairing (and the rescue), --ins-min / --ins-max / --ins-mean estimated from the pairs on the
//                 device   kiss_hip_fmi_insert_host (kiss --help-pairs)
//       --md      MD:Z: behind NM:i: on the mapped lines, written on the device   kiss_hip_fmi_md_host (kiss --help-sam)
//       --batch-reads N  with --sam: the file N reads (N pairs) at a time, cut on the device   kiss_hip_reads_parse_part_host
//                 (cli_batches.hpp; kiss --help-reads)
//       --sam-writer host|device  with --sam: the alignment lines built on the host (the default), or written on the device
//                 kiss_hip_fmi_sam_host (kiss --help-sam)
//       --bam FILE  with --sam: BAM to FILE ('-': stdout) in the place of the SAM lines; records and BGZF blocks written on the
//                 device   kiss_hip_fmi_bam_host, kiss_hip_bgzf_host (cli_bam.hpp; kiss --help-bam)
//       --bam-compress  with --bam: the BGZF blocks compressed on the device (DEFLATE)   kiss_hip_bgzf_deflate_host
//       --bam-sort  with --bam: the records of the whole file in coordinate order, sorted once on the device behind the last
//                 batch, SO:coordinate in the header   kiss_hip_bam_sort_host (cli_bam_sort.hpp; kiss --help-bam)
//       --bam-index  with --bam FILE --bam-sort: FILE.bai, the BAI index of the sorted file, built on the device and written
//                 behind FILE   kiss_hip_bai_host (cli_bam_index.hpp; kiss --help-bam)
//       --bam-markdup  with --bam FILE --bam-sort: FLAG 0x400 on the duplicate templates of the whole file, marked on the device
//                 directly before the sort   kiss_hip_bam_markdup_host (kiss --help-bam); --bam-markdup-min-qual Q
//   * -g / --generic with any of the three: the file is a text over the byte alphabet, byte for byte (no FASTA rule, no newline
//     stripping, no % 4): kiss_hip_suffix_sort_u8 (-k, -s ignored), kiss_hip_lcp_u8, kiss_hip_fmi8_build_host -> <file>.fmi8
//     (DESIGN.md 4.7), kiss_hip_fmi8_query_host.  One device, no lookup table, no mismatches.  The reference rejects -g.
// Input handling as utils/io.hpp:6-18 + suffix_sort.hpp:33: FASTA if the first byte is '>' (all records concatenated), else
// plain text lines; ACGT/acgt -> 0..3, every other character -> 4 % 4 = 0 (A).
#include "cli_reads.hpp"

namespace {

using namespace kiss_cli;

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
    if ((uint64_t)a.k >= bytes || (uint64_t)a.k >= scan_records(a.fasta).bounds.back()) return; // (the bases by the device parser's rule, without a device)
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

int fmindex_query_main(const Args &a)
{
    if (!a.seeds.empty()) { // (the text itself is not needed)
        Fmi f(a.sa_intv, 0);
        f.load(a.fasta + ".fmi");
        return map_reads(a, f.view_ex());
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
