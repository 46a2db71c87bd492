/*
 * kgx_sig_plan.h -- the host side of signature selection in key-range passes
 *                   (DESIGN.md §8.8): the rank of a letter, the planner that
 *                   cuts the key space into passes of at most B tuples, and
 *                   the arithmetic of the automatic budget.  No HIP in here:
 *                   tests/native/sig_plan_check.cpp drives it on the CPU.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "kgx.h"

namespace kgx {

/* ok_prot's 40 letters in ascending byte order: upper case before lower, so
 * the order of rank prefixes is the order of raw keys */
static const char kSigLetters[] = "ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy";
constexpr uint32_t kSigRanks = 40;
constexpr uint32_t kSigBins = kSigRanks * kSigRanks; /* two letters */
constexpr uint8_t kSigNoRank = 0xFF;
constexpr int kSigMaxDepth = 6;                       /* a bin at depth 6 is one key */
constexpr uint64_t kSigMaxPassTuples = 0x7FFFFFFFull; /* hipCUB counts items in an int */
constexpr uint64_t kSigAllKeys = ~0ull;               /* hi_key of the pass that is not planned: no key is all 0xFF */

/* byte -> rank among the 40 letters, kSigNoRank for every other byte */
inline void sig_rank_table(uint8_t table[256])
{
    std::fill(table, table + 256, kSigNoRank);
    for (uint32_t r = 0; r < kSigRanks; r++)
        table[(uint8_t)kSigLetters[r]] = (uint8_t)r;
}

/* keys lo_key <= raw_key < hi_key, which hold n_tuples tuples */
struct SigPass {
    uint64_t lo_key, hi_key, n_tuples;
};

/* counts[a * 40 + b] = the tuples whose key starts with the d letters of
 * `prefix` (its top d bytes; the rest are zero) followed by the letters of
 * rank a and b; returns KGX_OK or an error that ends the planning */
using SigCounter = std::function<int(uint64_t prefix, int d, uint64_t *counts)>;

/* the key whose letters d and d + 1 are those of `bin`, under `prefix` */
inline uint64_t sig_bin_key(uint64_t prefix, int d, uint32_t bin)
{
    return prefix | (uint64_t)(uint8_t)kSigLetters[bin / kSigRanks] << (8 * (7 - d)) |
           (uint64_t)(uint8_t)kSigLetters[bin % kSigRanks] << (8 * (6 - d));
}

/* Greedy packing of the bins, taken in ascending key order, into passes of
 * at most `budget` tuples: a bin that fits the open pass joins it, one that
 * does not closes it and opens the next, and one that alone exceeds the
 * budget is replaced by its 1,600 bins two letters deeper.  Any two
 * consecutive passes therefore hold more than `budget` tuples together (the
 * second one's first bin did not fit the first), so T tuples make at most
 * 2 T / budget + 1 passes.  A pass runs from its first bin's first key to
 * the end of its last bin: the passes are ascending and disjoint, and the
 * keys between them hold no tuple. */
class SigPlanner {
  public:
    SigPlanner(uint64_t budget, SigCounter count) : budget_(budget), count_(std::move(count)) {}

    /* KGX_OK; KGX_ERANGE when one key holds more than the budget (a set
     * cannot be split), with the k-mer and its count in error(); or the
     * counter's error */
    int plan(std::vector<SigPass> *out)
    {
        passes_.clear();
        open_ = false;
        const int rc = refine(0, 0);
        if (rc != KGX_OK)
            return rc;
        close();
        out->swap(passes_);
        return KGX_OK;
    }
    const std::string &error() const { return error_; }
    uint32_t count_calls() const { return calls_; }

  private:
    int refine(uint64_t prefix, int d)
    {
        std::vector<uint64_t> counts(kSigBins, 0);
        calls_++;
        const int rc = count_(prefix, d, counts.data());
        if (rc != KGX_OK)
            return rc;
        for (uint32_t bin = 0; bin < kSigBins; bin++) {
            const uint64_t c = counts[bin];
            if (c == 0)
                continue;
            const uint64_t lo = sig_bin_key(prefix, d, bin);
            if (c > budget_) {
                if (d == kSigMaxDepth) {
                    std::string kmer(8, '?');
                    for (int j = 0; j < 8; j++)
                        kmer[j] = (char)(lo >> (8 * (7 - j)));
                    error_ = "signature selection: k-mer " + kmer + " holds " + std::to_string(c) +
                             " tuples, more than max_pass_tuples = " + std::to_string(budget_) +
                             "; a set cannot be split";
                    return KGX_ERANGE;
                }
                const int rc2 = refine(lo, d + 2);
                if (rc2 != KGX_OK)
                    return rc2;
                continue;
            }
            if (open_ && cur_.n_tuples + c > budget_)
                close();
            if (!open_) {
                open_ = true;
                cur_ = {lo, 0, 0};
            }
            cur_.n_tuples += c;
            cur_.hi_key = lo + (1ull << (8 * (6 - d))); /* a letter is below 0x7A: the byte does not carry */
        }
        return KGX_OK;
    }
    void close()
    {
        if (open_)
            passes_.push_back(cur_);
        open_ = false;
    }

    uint64_t budget_;
    SigCounter count_;
    std::vector<SigPass> passes_;
    SigPass cur_{};
    bool open_ = false;
    uint32_t calls_ = 0;
    std::string error_;
};

/* ---- the automatic budget --------------------------------------------------
 * What a pass of P tuples allocates, in bytes per tuple (kgx_sig.hip):
 *   32  the tuples, {key, value} of 8 bytes each, twice: the radix sorts'
 *       input and output (the copy also holds the set heads and starts)
 *   16  the sorts' scratch: hipCUB keeps one more copy of keys and values
 *   13  per set, and a set may be a single tuple: best function 4, its count
 *       4, the keep flag 1, the kept set's id 4
 *    1  the two lists of larger sets: 4 / 17 + 4 / 4097 bytes, rounded up
 * and once, whatever P: the scratch's histograms, the counters, the 1,600
 * bins and the allocator's rounding of some twenty buffers. */
constexpr uint64_t kSigPassBytesPerTuple = 32 + 16 + 13 + 1;
constexpr uint64_t kSigRecordBytes = 40; /* sizeof(kgx_sig_record) */
constexpr uint64_t kSigFixedBytes = 64ull << 20;

/* The largest pass for `free_bytes` of device memory left after the uploads
 * and a corpus of `n_windows` windows.  The records of all passes stay on the
 * device beside the pass buffers: at most one per set, so at most one per
 * window, 40 bytes each.  That worst case is set aside whenever it leaves the
 * passes at least half of the memory; the rest is divided by the bytes per
 * tuple.  (With n_windows <= the result a single pass holds everything, its
 * records included.)  Where the worst case would take more than half, no
 * split serves every corpus: one that keeps a record per window does not fit
 * at all, so the passes get half -- their 62 bytes per tuple and the records'
 * 40 are of one size, and a corpus that fails the even split is within a
 * factor of two of fitting under no split.  A record buffer that cannot be
 * had is KGX_ENOMEM in any case.  Monotone in free_bytes; in
 * [1, kSigMaxPassTuples]. */
inline uint64_t sig_auto_budget(uint64_t free_bytes, uint64_t n_windows)
{
    const uint64_t avail = free_bytes > kSigFixedBytes ? free_bytes - kSigFixedBytes : 0;
    const uint64_t records = n_windows > avail / kSigRecordBytes ? avail : n_windows * kSigRecordBytes;
    const uint64_t passes = std::max(avail / 2, avail - records);
    return std::min(std::max<uint64_t>(passes / kSigPassBytesPerTuple, 1), kSigMaxPassTuples);
}

}  // namespace kgx
