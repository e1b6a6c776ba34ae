// cli_batches.hpp -- `kiss fmindex_query --seeds READS --sam --batch-reads N`: a read file of any size fed to the part call
// (include/kiss_hip_reads_part.h) a chunk at a time.  A ChunkReader holds the bytes read and not yet consumed;
// ready(N) reads on until N whole records stand at their head or the file's end is among them, take(K) parses the first K and takes
// their bytes off.  The record boundary is found by the part call, on the device; the host looks at no byte but the names'.
// A template over the part call, which is the only thing here that needs the library: kiss_hip_reads_part.h gives types and
// constants alone, so the reader is tested without a device (tests/test_cli_batches.py, with a host cut in the call's place).
//   part(raw, bytes, format, final, max_records, codes, qual, bases_capacity, read_index, name_off, name_len, reads_capacity, report)
// returns KISS_HIP_OK or KISS_HIP_E_INVALID as kiss_hip_reads_parse_part_host does and throws on every other answer.
#pragma once
#include "cli_format.hpp"
#include "../../../include/kiss_hip_reads_part.h"

namespace kiss_cli {

inline const char *fastq_bad_kind(uint32_t kind)
{
    static const char *const kinds[] = {"", "its first line does not start with '@'", "its third line does not start with '+'",
                                        "its sequence and its quality string differ in length", "the file ends inside it"};
    return kinds[kind % 5];
}

template <class Part> class ChunkReader {
  public:
    // format: the KISS_HIP_READS_* asked for (AUTO is resolved by the first records taken); chunk_bytes: what one look at the file reads
    ChunkReader(const std::string &path, int format, uint64_t chunk_bytes, bool with_names, Part part)
        : path_(path), in_(path, std::ios::binary), format_(format), chunk_(chunk_bytes ? chunk_bytes : 1), with_names_(with_names), part_(part)
    {
        if (!in_) throw std::runtime_error("cannot open " + path);
        buf_.reserve(1); // (a pointer that is not NULL)
    }
    const std::string &path() const { return path_; }
    uint64_t first() const { return first_; } // the records taken so far: the file-wide number of the next one
    int format() const { return format_; }

    // The whole records at the head of what is left of the file, up to max_records (>= 1) of them.  Fewer than max_records: the
    // file ends behind them; 0: nothing is left but empty lines.  Reads chunk_bytes more, then twice that, and so on, until the
    // part call finds max_records or `final` is established: a record longer than a chunk is no error.  A bad FASTQ record among
    // the first max_records stops here, under its number in the file.
    uint64_t ready(uint64_t max_records)
    {
        if (done_) return 0;
        uint64_t step = chunk_;
        for (bool more = buf_.size() < chunk_;; more = true, step *= 2) {
            if (more && !final_) read_on(step);
            size(max_records);
            if (rep_.records == max_records || final_) return rep_.records;
        }
    }

    // The first K records (1 <= K <= what ready() answered) parsed, with_names with their names: the file's, or the number of
    // the read in the file.  Their bytes leave the buffer; the tail stays in front of what is read next.
    ReadFile take(uint64_t K)
    {
        if (!sized_ || rep_.records != K) size(K);
        if (rep_.records != K) throw std::logic_error("ChunkReader::take: " + std::to_string(K) + " records are not ready");
        ReadFile f;
        const uint64_t bases = rep_.parsed.bases, reads = rep_.parsed.reads;
        std::vector<uint64_t> off(reads + 1, 0);
        std::vector<uint32_t> len(reads + 1, 0);
        f.reads.resize(bases + 1);
        f.qual.resize(bases + 1);
        f.ridx.assign(reads + 1, 0);
        const int rc = part_(buf_.data(), buf_.size(), format_, final_ ? 1 : 0, K, f.reads.data(), f.qual.data(), bases, f.ridx.data(),
                             with_names_ ? off.data() : nullptr, with_names_ ? len.data() : nullptr, reads, &rep_);
        sized_ = false;
        if (rc != KISS_HIP_OK || rep_.records != K || rep_.parsed.reads != reads || rep_.parsed.bases != bases || rep_.bytes_used > buf_.size())
            throw std::runtime_error("fmindex_query --seeds: the part call refused a chunk of " + path_ + " that it had sized");
        if (rep_.parsed.empty_reads)
            throw std::runtime_error("fmindex_query --seeds: read " + std::to_string(first_ + rep_.parsed.first_empty) + " of " + path_ +
                                     " has no bases (" + std::to_string(rep_.parsed.empty_reads) + " such reads in its batch)");
        f.has_qual = rep_.parsed.has_qual != 0;
        f.reads.resize(bases);
        f.qual.resize(f.has_qual ? bases : 0);
        for (uint64_t q = 0; q < reads && with_names_; q++)
            f.names.push_back(len[q] ? std::string((const char *)buf_.data() + off[q], len[q]) : std::to_string(first_ + q));
        format_ = (int)rep_.parsed.format;
        first_ += rep_.records;
        done_ = final_ && rep_.records == rep_.records_complete;
        buf_.erase(buf_.begin(), buf_.begin() + (std::ptrdiff_t)rep_.bytes_used);
        buf_.reserve(1);
        return f;
    }

  private:
    // `want` bytes more behind the tail; final_ as soon as the file's end is in the buffer, before anything is cut
    void read_on(uint64_t want)
    {
        const size_t had = buf_.size();
        buf_.resize(had + want);
        in_.read(reinterpret_cast<char *>(buf_.data() + had), (std::streamsize)want);
        buf_.resize(had + (size_t)in_.gcount());
        buf_.reserve(1);
        final_ = !in_ || in_.peek() == EOF;
    }
    // the size call: rep_ says what max_records of the buffer's records need
    void size(uint64_t max_records)
    {
        rep_ = kiss_hip_reads_part_report{};
        uint64_t ridx0 = 0;
        const int rc = part_(buf_.data(), buf_.size(), format_, final_ ? 1 : 0, max_records, nullptr, nullptr, 0, &ridx0, nullptr, nullptr, 0, &rep_);
        if (rc == KISS_HIP_E_INVALID && rep_.parsed.bad_records)
            throw std::runtime_error("fmindex_query --seeds: " + path_ + " is no FASTQ file: the first bad record is record " +
                                     std::to_string(first_ + rep_.parsed.first_bad) + ": " + fastq_bad_kind(rep_.parsed.first_bad_kind));
        if (rc == KISS_HIP_E_INVALID && !(rep_.parsed.reads || rep_.parsed.bases))
            throw std::runtime_error("fmindex_query --seeds: the part call refused a chunk of " + path_);
        sized_ = true;
    }

    std::string path_;
    std::ifstream in_;
    std::vector<uint8_t> buf_;
    int format_;
    uint64_t chunk_, first_ = 0;
    bool with_names_, final_ = false, done_ = false, sized_ = false;
    kiss_hip_reads_part_report rep_{};
    Part part_;
};

} // namespace kiss_cli
