/*
 * kgx_sig.hip -- signature k-mer selection on the device: labelled proteins
 *                in, kept 8-mers with function, median offset and weight out
 *                (build_signature_kmers.cc: load_sequence :572-633,
 *                process_set :663-710, compute_weight_of_signature :841-853,
 *                write_hashtable :860-898).  DESIGN.md §8.8 states the rules.
 *
 *   passes    a corpus of more tuples than one pass may hold (max_pass_tuples)
 *             is selected in passes over ascending, disjoint ranges of raw
 *             key, planned on the host (kgx_sig_plan.h) from counts of the
 *             windows by their leading letters (count: as emit walks them,
 *             1,600 bins per workgroup in LDS).  Every stage below up to the
 *             records runs per pass; NSF, KS and the weights follow the last
 *   emit      one thread per residue position; the 8 bytes of its window are
 *             checked against a 256-byte LDS table (the ranks of the 40
 *             letters of ok_prot) and valid windows of labelled sequences
 *             whose key lies in the pass's range are written, compacted, as
 *             {raw key (8 bytes big-endian), n << 32 | sequence}
 *   order     two stable hipCUB radix sorts: by n, then by raw key -- a set
 *             (all tuples of one key) is contiguous and ordered by offset,
 *             so its median is one read
 *   segment   by set size: a thread per set up to kSmallSet tuples, a wave
 *             per set up to kWaveSet, a workgroup per larger set.  Majority
 *             vote (MJRTY) over the tuples' functions, recount, the keep
 *             test in the reference's float/double form, atomicOr of the
 *             kept sets' sequences into a bitmap
 *   popcount  of the bitmap: sequences with a signature (NSF)
 *   records   kept sets compacted in set (= ascending key) order, each with
 *             its base-20 code, median and weight (double log)
 *   image     the storable records handed, on the device, to the insert
 *             kgx_image_build uses (kgx_synth.hip)
 */
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "kgx.h"
#include "kgx_device.h"
#include "kgx_rt.h"
#include "kgx_sig_plan.h"

namespace kgx {

constexpr uint32_t kSmallSet = 16;   /* thread per set up to here */
constexpr uint32_t kWaveSet = 4096;  /* wave per set up to here, a workgroup beyond */
constexpr int kSigStages = KGX_SIG_STAGES;

/* build_signature_kmers.cc:862-865, in list order (it is not sorted) */
static const uint64_t kBuilderPrimes[] = {3769, 6337, 12791, 24571, 51043, 101533, 206933, 400187, 821999,
                                          2000003, 4000037, 8000009, 16000057, 32000011, 64000031, 128000003,
                                          248000009, 508000037, 1073741824, 1400303159, 2147483648ULL, 1190492993,
                                          3559786523ULL, 6461346257ULL};

/* the first listed size above 3 * n_kept; 0 when the list has none */
static uint64_t builder_num_sigs(uint64_t n_kept)
{
    for (uint64_t p : kBuilderPrimes)
        if (p > 3 * n_kept)
            return p;
    return 0;
}

/* ---- emit ---------------------------------------------------------------- */

/* the sequence holding residue position g, given off[lo] <= g < off[hi]:
 * the last s with off[s] <= g (empty sequences share an offset with their
 * successor) */
__device__ __forceinline__ uint32_t seq_of(const uint64_t *__restrict__ off, uint32_t lo, uint32_t hi, uint64_t g)
{
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= g)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

/* byte -> rank among the 40 letters of ok_prot in ascending byte order (the
 * 20 residues, then the same in lower case: clearing bit 5 maps 'a'..'z' onto
 * 'A'..'Z' and nothing else onto them), kSigNoRank for every other byte: the
 * device's form of sig_rank_table (kgx_sig_plan.h) */
__device__ __forceinline__ uint8_t sig_rank(uint32_t c)
{
    const uint32_t r = residue_code(c & ~0x20u);
    return r < 20u ? (uint8_t)(r + ((c & 0x20u) ? 20u : 0u)) : kSigNoRank;
}

/* What emit and count share: a tile of 256 residue positions and each
 * thread's window of it. */
struct SigTile {
    uint8_t rank[256];
    uint8_t tile[256 + 8];
    uint32_t tile_seq[2]; /* the sequences of the tile's first and last position */
};

__device__ __forceinline__ void sig_tile_init(SigTile &sh) { sh.rank[threadIdx.x] = sig_rank(threadIdx.x); }

/* Loads the tile at g0 and decides thread t's window, at position g0 + t: a
 * tuple iff it lies in a labelled sequence and its 8 bytes are letters.
 * Every thread of the workgroup calls it; it starts with a barrier (the table
 * on the first round, the last round's tile after). */
__device__ __forceinline__ bool sig_tile_window(SigTile &sh, const uint8_t *__restrict__ res, uint64_t total,
                                                const uint64_t *__restrict__ off, uint32_t n_seq,
                                                const int32_t *__restrict__ seq_fn, uint64_t g0, uint64_t &key,
                                                uint64_t &val)
{
    const uint32_t t = threadIdx.x;
    __syncthreads();
    for (uint32_t i = t; i < 256 + 8; i += 256)
        sh.tile[i] = g0 + i < total ? res[g0 + i] : 0;
    /* two searches of the whole offset array per tile; the threads then search between them */
    if (t == 0 || t == 255)
        sh.tile_seq[t >> 7] = seq_of(off, 0, n_seq, std::min(g0 + t, total - 1));
    __syncthreads();
    const uint64_t g = g0 + t;
    bool valid = false;
    key = 0;
    val = 0;
    if (g < total) {
        const uint32_t s = seq_of(off, sh.tile_seq[0], sh.tile_seq[1] + 1, g);
        const uint64_t end = off[s + 1];
        if (seq_fn[s] >= 0 && g + 8 <= end) {
            valid = true;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) {
                const uint32_t c = sh.tile[t + j];
                valid = valid && sh.rank[c] != kSigNoRank;
                key = key << 8 | c;
            }
            val = (end - g) << 32 | s;
        }
    }
    return valid;
}

/* the tuples with lo <= key < hi, compacted */
__global__ __launch_bounds__(256) void sig_emit_kernel(const uint8_t *__restrict__ res, uint64_t total,
                                                       const uint64_t *__restrict__ off, uint32_t n_seq,
                                                       const int32_t *__restrict__ seq_fn, uint64_t lo, uint64_t hi,
                                                       uint64_t *keys, uint64_t *vals, uint64_t cap,
                                                       unsigned long long *n_out)
{
    __shared__ SigTile sh;
    __shared__ uint32_t wave_n[4];
    __shared__ unsigned long long block_base;
    const uint32_t t = threadIdx.x;
    sig_tile_init(sh);
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256; g0 < total; g0 += (uint64_t)gridDim.x * 256) {
        uint64_t key, val;
        const bool valid = sig_tile_window(sh, res, total, off, n_seq, seq_fn, g0, key, val) && key >= lo && key < hi;
        const uint64_t m = __ballot(valid);
        if (lane_id() == 0)
            wave_n[t >> 6] = (uint32_t)__popcll(m);
        __syncthreads();
        if (t == 0)
            block_base = atomicAdd(n_out, (unsigned long long)(wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3]));
        __syncthreads();
        uint64_t j = block_base + lanes_below(m);
        for (uint32_t w = 0; w < (t >> 6); w++)
            j += wave_n[w];
        if (valid && j < cap) {
            keys[j] = key;
            vals[j] = val;
        }
    }
}

/* Planning: among the tuples whose key starts with the d letters of `prefix`
 * (its top d bytes), how many continue with each pair of letters.  The 1,600
 * bins are the workgroup's own in LDS; a window costs one LDS atomic and no
 * global one, and the workgroup adds its non-zero bins to `bins` once, after
 * its last tile. */
__global__ __launch_bounds__(256) void sig_count_kernel(const uint8_t *__restrict__ res, uint64_t total,
                                                        const uint64_t *__restrict__ off, uint32_t n_seq,
                                                        const int32_t *__restrict__ seq_fn, uint64_t prefix,
                                                        uint32_t d, unsigned long long *bins)
{
    __shared__ SigTile sh;
    __shared__ uint32_t hist[kSigBins]; /* a workgroup sees fewer than 2^32 positions */
    const uint32_t t = threadIdx.x;
    sig_tile_init(sh);
    for (uint32_t i = t; i < kSigBins; i += 256)
        hist[i] = 0;
    const uint32_t rest = 64 - 8 * d; /* d <= 6: the bits below the prefix */
    for (uint64_t g0 = (uint64_t)blockIdx.x * 256; g0 < total; g0 += (uint64_t)gridDim.x * 256) {
        uint64_t key, val;
        const bool valid = sig_tile_window(sh, res, total, off, n_seq, seq_fn, g0, key, val);
        if (valid && (d == 0 || (key ^ prefix) >> rest == 0)) {
            const uint32_t a = sh.rank[(key >> (rest - 8)) & 0xFFu], b = sh.rank[(key >> (rest - 16)) & 0xFFu];
            atomicAdd(&hist[a * kSigRanks + b], 1u);
        }
    }
    __syncthreads();
    for (uint32_t i = t; i < kSigBins; i += 256)
        if (hist[i])
            atomicAdd(&bins[i], (unsigned long long)hist[i]);
}

/* ---- sets ------------------------------------------------------------------ */

__global__ void sig_heads_kernel(const uint64_t *__restrict__ keys, uint32_t n, uint8_t *head)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n)
        head[i] = i == 0 || keys[i] != keys[i - 1];
}

/* MJRTY summaries merge: what is left of each side after pairing off
 * unequal elements is `n` copies of `c` */
struct Vote {
    int32_t c;
    uint32_t n;
};
__device__ __forceinline__ Vote vote_add(Vote a, int32_t f)
{
    if (a.n == 0)
        return {f, 1u};
    return a.c == f ? Vote{a.c, a.n + 1} : Vote{a.c, a.n - 1};
}
__device__ __forceinline__ Vote vote_merge(Vote a, Vote b)
{
    if (a.c == b.c)
        return {a.c, a.n + b.n};
    return a.n >= b.n ? Vote{a.c, a.n - b.n} : Vote{b.c, b.n - a.n};
}
__device__ __forceinline__ Vote vote_wave(Vote v)
{
    for (int d = 32; d; d >>= 1) {
        Vote o;
        o.c = __shfl_down(v.c, d);
        o.n = (uint32_t)__shfl_down((int)v.n, d);
        v = vote_merge(v, o);
    }
    return v; /* lane 0 holds the wave's */
}
__device__ __forceinline__ uint32_t sum_wave(uint32_t x)
{
    for (int d = 32; d; d >>= 1)
        x += (uint32_t)__shfl_down((int)x, d);
    return x; /* lane 0 */
}

/* process_set's test, build_signature_kmers.cc:672-682: thresh is a float
 * holding float(count) * 0.8 taken in double */
__device__ __forceinline__ bool sig_keep(uint32_t best, uint32_t count)
{
    const float thresh = (float)((double)(float)count * 0.8);
    return !((float)best < thresh);
}

struct SetOut {
    int32_t *best;
    uint32_t *n_best;
    uint8_t *keep;
};

__device__ __forceinline__ int32_t fn_of(const uint64_t *__restrict__ vals, const int32_t *__restrict__ seq_fn,
                                         uint32_t i)
{
    return seq_fn[(uint32_t)vals[i]];
}

/* sequence q has a signature.  A sequence is marked once per tuple of a kept
 * set, so the bit is nearly always set already: look before the atomic */
__device__ __forceinline__ void mark_seq(uint32_t *bitmap, uint32_t q)
{
    const uint32_t bit = 1u << (q & 31u);
    if (!(__atomic_load_n(&bitmap[q >> 5], __ATOMIC_RELAXED) & bit))
        atomicOr(&bitmap[q >> 5], bit);
}

/* every set: the small ones are decided here, the others are listed */
__global__ __launch_bounds__(256) void sig_small_kernel(const uint32_t *__restrict__ starts, uint32_t n_sets,
                                                        const uint64_t *__restrict__ vals,
                                                        const int32_t *__restrict__ seq_fn, SetOut out,
                                                        uint32_t *bitmap, uint32_t *wave_list, uint32_t *block_list,
                                                        uint32_t *n_lists)
{
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_sets; s += gridDim.x * blockDim.x) {
        const uint32_t b = starts[s], cnt = starts[s + 1] - b;
        if (cnt > kWaveSet) {
            block_list[atomicAdd(&n_lists[1], 1u)] = s;
            continue;
        }
        if (cnt > kSmallSet) {
            wave_list[atomicAdd(&n_lists[0], 1u)] = s;
            continue;
        }
        Vote v{-1, 0};
        for (uint32_t i = 0; i < cnt; i++)
            v = vote_add(v, fn_of(vals, seq_fn, b + i));
        uint32_t nb = 0;
        for (uint32_t i = 0; i < cnt; i++)
            nb += fn_of(vals, seq_fn, b + i) == v.c;
        const bool keep = sig_keep(nb, cnt);
        out.best[s] = v.c;
        out.n_best[s] = nb;
        out.keep[s] = keep;
        if (keep)
            for (uint32_t i = 0; i < cnt; i++) {
                mark_seq(bitmap, (uint32_t)vals[b + i]);
            }
    }
}

/* a wave per listed set */
__global__ __launch_bounds__(256) void sig_wave_kernel(const uint32_t *__restrict__ starts,
                                                       const uint32_t *__restrict__ list,
                                                       const uint32_t *__restrict__ n_list,
                                                       const uint64_t *__restrict__ vals,
                                                       const int32_t *__restrict__ seq_fn, SetOut out,
                                                       uint32_t *bitmap)
{
    const uint32_t n = *n_list, lane = lane_id();
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); k < n; k += waves) {
        const uint32_t s = list[k], b = starts[s], cnt = starts[s + 1] - b;
        Vote v{-1, 0};
        for (uint32_t i = lane; i < cnt; i += 64)
            v = vote_add(v, fn_of(vals, seq_fn, b + i));
        v = vote_wave(v);
        const int32_t best = __shfl(v.c, 0);
        uint32_t nb = 0;
        for (uint32_t i = lane; i < cnt; i += 64)
            nb += fn_of(vals, seq_fn, b + i) == best;
        nb = (uint32_t)__shfl((int)sum_wave(nb), 0);
        const bool keep = sig_keep(nb, cnt);
        if (lane == 0) {
            out.best[s] = best;
            out.n_best[s] = nb;
            out.keep[s] = keep;
        }
        if (keep)
            for (uint32_t i = lane; i < cnt; i += 64) {
                mark_seq(bitmap, (uint32_t)vals[b + i]);
            }
    }
}

/* a workgroup (4 waves) per listed set, its tuples strided over the threads;
 * the only LDS is the four waves' summaries */
__global__ __launch_bounds__(256) void sig_block_kernel(const uint32_t *__restrict__ starts,
                                                        const uint32_t *__restrict__ list,
                                                        const uint32_t *__restrict__ n_list,
                                                        const uint64_t *__restrict__ vals,
                                                        const int32_t *__restrict__ seq_fn, SetOut out,
                                                        uint32_t *bitmap)
{
    __shared__ Vote wv[4];
    __shared__ uint32_t wn[4];
    const uint32_t n = *n_list, t = threadIdx.x, lane = lane_id(), w = t >> 6;
    for (uint32_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint32_t s = list[k], b = starts[s], cnt = starts[s + 1] - b;
        Vote v{-1, 0};
        for (uint32_t i = t; i < cnt; i += 256)
            v = vote_add(v, fn_of(vals, seq_fn, b + i));
        v = vote_wave(v);
        if (lane == 0)
            wv[w] = v;
        __syncthreads();
        const int32_t best = vote_merge(vote_merge(wv[0], wv[1]), vote_merge(wv[2], wv[3])).c;
        uint32_t nb = 0;
        for (uint32_t i = t; i < cnt; i += 256)
            nb += fn_of(vals, seq_fn, b + i) == best;
        nb = sum_wave(nb);
        if (lane == 0)
            wn[w] = nb;
        __syncthreads();
        nb = wn[0] + wn[1] + wn[2] + wn[3];
        const bool keep = sig_keep(nb, cnt);
        if (t == 0) {
            out.best[s] = best;
            out.n_best[s] = nb;
            out.keep[s] = keep;
        }
        if (keep)
            for (uint32_t i = t; i < cnt; i += 256) {
                mark_seq(bitmap, (uint32_t)vals[b + i]);
            }
        __syncthreads(); /* wv / wn are rewritten by the next set */
    }
}

__global__ __launch_bounds__(256) void sig_popcount_kernel(const uint32_t *__restrict__ bitmap, uint32_t n_words,
                                                           unsigned long long *total)
{
    uint32_t c = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += gridDim.x * blockDim.x)
        c += (uint32_t)__popc(bitmap[i]);
    c = sum_wave(c);
    if (lane_id() == 0 && c)
        atomicAdd(total, (unsigned long long)c);
}

/* ---- records --------------------------------------------------------------- */

/* KmerEncoder::encoded_aa_kmer: upper case only; anything else is not storable */
__device__ __forceinline__ uint64_t sig_code(uint64_t raw)
{
    uint64_t code = 0;
    bool ok = true;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint32_t c = residue_code((uint32_t)(raw >> (8 * j)) & 0xFFu);
        ok = ok && c < 20u;
        code = code * 20 + c;
    }
    return ok ? code : EMPTY_KEY;
}

/* compute_weight_of_signature, build_signature_kmers.cc:841-853: float
 * locals; the first quotient in double, the second in float; both logs the
 * double one */
__device__ __forceinline__ float sig_weight(float NSF, float KS, float NSi, float NFj, float NSiFj)
{
    const double a = log(((double)NSiFj + 1.0) / ((double)(NSi - NSiFj) + 1.0));
    const float q = (NSF - NFj + KS) / (NFj + KS);
    return (float)(a + log((double)q));
}

/* The records of one pass's kept sets.  kFinal: the pass is the only one, NSF
 * and KS (= n_kept) are known, and the weights and the storable count are
 * taken here.  Otherwise both wait for sig_weights_kernel after the last
 * pass, and function_wt is left 0. */
template <bool kFinal>
__global__ __launch_bounds__(256) void sig_records_kernel(const uint32_t *__restrict__ kept, uint32_t n_kept,
                                                          const uint32_t *__restrict__ starts,
                                                          const uint64_t *__restrict__ keys,
                                                          const uint64_t *__restrict__ vals, SetOut sets,
                                                          const uint32_t *__restrict__ n_fn, float NSF,
                                                          kgx_sig_record *recs, unsigned long long *n_storable)
{
    uint32_t storable = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_kept; r += gridDim.x * blockDim.x) {
        const uint32_t s = kept[r], b = starts[s], cnt = starts[s + 1] - b;
        kgx_sig_record o;
        o.raw_key = keys[b];
        o.code = sig_code(o.raw_key);
        o.function_index = sets.best[s];
        o.n_tuples = cnt;
        o.n_best = sets.n_best[s];
        o.median_offset = (int32_t)(vals[b + cnt / 2] >> 32);
        o.function_wt = 0.0f;
        if (kFinal)
            o.function_wt =
                sig_weight(NSF, (float)n_kept, (float)cnt, (float)n_fn[o.function_index], (float)o.n_best);
        recs[r] = o;
        reinterpret_cast<uint32_t *>(recs + r)[9] = 0; /* the struct's tail padding: no stale bytes reach the host */
        storable += o.code <= MAX_ENCODED;
    }
    if (!kFinal)
        return;
    storable = sum_wave(storable); /* one add per wave: same-address atomics serialise */
    if (lane_id() == 0 && storable)
        atomicAdd(n_storable, (unsigned long long)storable);
}

/* after the last of several passes: the weights of n records (one pass's
 * share of the KS kept ones) and the storable among them */
__global__ __launch_bounds__(256) void sig_weights_kernel(kgx_sig_record *recs, uint64_t n,
                                                          const uint32_t *__restrict__ n_fn, float NSF, float KS,
                                                          unsigned long long *n_storable)
{
    uint32_t storable = 0; /* a thread sees fewer than 2^32 records */
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (uint64_t)gridDim.x * blockDim.x) {
        const kgx_sig_record o = recs[r];
        recs[r].function_wt =
            sig_weight(NSF, KS, (float)o.n_tuples, (float)n_fn[o.function_index], (float)o.n_best);
        storable += o.code <= MAX_ENCODED;
    }
    storable = sum_wave(storable);
    if (lane_id() == 0 && storable)
        atomicAdd(n_storable, (unsigned long long)storable);
}

/* n records as the insert's entry arrays, from entry `base` on */
__global__ void sig_entries_kernel(const kgx_sig_record *__restrict__ recs, uint64_t n, uint64_t base, uint64_t *keys,
                                   int32_t *fi, int32_t *otu, uint16_t *avg, float *wt)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n)
        return;
    const uint64_t e = base + r;
    keys[e] = recs[r].code;
    fi[e] = recs[r].function_index;
    otu[e] = -1;
    avg[e] = (uint16_t)recs[r].median_offset; /* truncates, as insert_kmer's unsigned short parameter */
    wt[e] = recs[r].function_wt;
}

static inline dim3 sig_grid(uint64_t n, uint32_t per_block = 256, uint32_t cap = 8192)
{
    return dim3((uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, cap)));
}

}  // namespace kgx

using namespace kgx;

static_assert(sizeof(kgx_sig_record) == 40, "kgx_sig_record: 36 bytes of fields, 4 of tail padding");

static_assert(sizeof(kgx_sig_record) == kSigRecordBytes, "the budget counts 40 bytes per record");

struct kgx_sig {
    int device = -1;
    kgx_sig_stats stats{};
    /* the stats.n_kept records in ascending raw_key order: the kept sets of
     * pass i, recs[i] of them (fewer than 2^31), are chunk[i].  A pass's
     * records are allocated when their number is known, so nothing is ever
     * copied to make room and the records take 40 bytes each, no more. */
    std::vector<DevBuf> chunk;
    std::vector<kgx_sig_pass> passes; /* those that held a tuple; chunk[i] belongs to passes[i] */
    std::vector<kgx_sig_record> host;
    bool host_valid = false;
    float stage_ms[kSigStages] = {};
};

/* an allocation that does not fit is KGX_ENOMEM, not a device error */
#define SIG_ALLOC(buf, bytes)                                                                       \
    do {                                                                                            \
        if ((buf).reserve(bytes) != hipSuccess) {                                                   \
            (void)hipGetLastError();                                                                \
            return fail(KGX_ENOMEM, "signature selection: the corpus does not fit the device (" #buf ")"); \
        }                                                                                           \
    } while (0)

namespace {

enum { kUpload = 0, kEmit, kOrder, kSegment, kRecords };

/* stage times: the time between two marks goes to the stage the later one
 * names, summed over the passes */
struct StageClock {
    std::vector<hipEvent_t> e; /* e[0] starts the next lap */
    std::vector<int> stage;    /* stage[i]: of the lap that ends at e[i] */
    float *ms;
    explicit StageClock(float *out) : ms(out) {}
    StageClock(const StageClock &) = delete;
    ~StageClock()
    {
        for (hipEvent_t x : e)
            (void)hipEventDestroy(x);
    }
    int mark(int s)
    {
        hipEvent_t x;
        HIP_TRY(hipEventCreate(&x));
        e.push_back(x);
        stage.push_back(s);
        HIP_TRY(hipEventRecord(x, nullptr));
        return KGX_OK;
    }
    /* adds the laps marked so far; the last mark starts the next lap */
    int flush()
    {
        if (e.empty())
            return KGX_OK;
        HIP_TRY(hipEventSynchronize(e.back()));
        for (size_t i = 1; i < e.size(); i++) {
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, e[i - 1], e[i]));
            ms[stage[i]] += t;
        }
        for (size_t i = 0; i + 1 < e.size(); i++)
            (void)hipEventDestroy(e[i]);
        e.erase(e.begin(), e.end() - 1);
        stage.erase(stage.begin(), stage.end() - 1);
        return KGX_OK;
    }
};

/* one selection: what lives across its passes */
struct SigRun {
    kgx_sig *S;
    uint64_t total = 0; /* residues */
    uint32_t n_seq = 0, max_len = 0, n_words = 0;
    DevBuf res, off, fn, nfn, cnt, bins, bitmap; /* the corpus, the counters, the planner's bins, NSF's bits */
    DevBuf kA, vA, kB, vB, tmp, best, nbest, keep, lists, kept; /* a pass's; they grow to the largest pass */
    StageClock clock;
    explicit SigRun(kgx_sig *s) : S(s), clock(s->stage_ms) {}
    /* cnt: tuples, NSF, storable | the two list lengths */
    unsigned long long *n_tup() const { return cnt.as<unsigned long long>(); }
    unsigned long long *n_sf() const { return n_tup() + 1; }
    unsigned long long *n_stor() const { return n_tup() + 2; }
    uint32_t *n_lists() const { return reinterpret_cast<uint32_t *>(n_tup() + 3); }
};

/* the planner's counter on the device: one launch per call */
int sig_count(SigRun &R, uint64_t prefix, int d, uint64_t *counts)
{
    HIP_TRY(hipMemset(R.bins.p, 0, kSigBins * 8));
    hipLaunchKernelGGL(sig_count_kernel, sig_grid(R.total, 256, 2048), dim3(256), 0, nullptr, R.res.as<uint8_t>(),
                       R.total, R.off.as<uint64_t>(), R.n_seq, R.fn.as<int32_t>(), prefix, (uint32_t)d,
                       R.bins.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(counts, R.bins.p, kSigBins * 8, hipMemcpyDeviceToHost));
    return KGX_OK;
}

/* One pass: the tuples with lo <= key < hi through emit, order, segment and
 * records.  cap: room for its tuples -- their exact number when the pass was
 * planned.  only: there is no other pass, so NSF and KS are this pass's and
 * its records are final; otherwise the weights wait for the last pass. */
int sig_pass(SigRun &R, uint64_t lo, uint64_t hi, uint64_t cap, bool planned, bool last, bool only)
{
    kgx_sig_stats &st = R.S->stats;
    int rc;
    HIP_TRY(hipMemset(R.cnt.p, 0, 4 * 8));

    /* emit */
    SIG_ALLOC(R.kA, cap * 8);
    SIG_ALLOC(R.vA, cap * 8);
    DevBuf &kA = R.kA, &vA = R.vA, &kB = R.kB, &vB = R.vB, &tmp = R.tmp;
    hipLaunchKernelGGL(sig_emit_kernel, sig_grid(R.total), dim3(256), 0, nullptr, R.res.as<uint8_t>(), R.total,
                       R.off.as<uint64_t>(), R.n_seq, R.fn.as<int32_t>(), lo, hi, kA.as<uint64_t>(), vA.as<uint64_t>(),
                       cap, R.n_tup());
    HIP_TRY(hipGetLastError());
    unsigned long long T = 0;
    HIP_TRY(hipMemcpy(&T, R.n_tup(), 8, hipMemcpyDeviceToHost));
    if (T > cap && !planned)
        return fail(KGX_EDEVICE, "signature selection: more tuples than windows");
    if (planned && T != cap)
        return fail(KGX_EDEVICE, "signature selection: a pass planned for " + std::to_string(cap) + " tuples emitted " +
                                     std::to_string(T));
    st.n_tuples += T;
    if (last)
        R.res.release();
    if ((rc = R.clock.mark(kEmit)))
        return rc;
    if (T == 0)
        return KGX_OK;

    /* order: by n (bits 32.. of the value), then by key; both stable */
    SIG_ALLOC(kB, T * 8);
    SIG_ALLOC(vB, T * 8);
    int n_bits = 1;
    while (n_bits < 32 && (R.max_len >> n_bits))
        n_bits++;
    size_t tb1 = 0, tb2 = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb1, vA.as<uint64_t>(), vB.as<uint64_t>(), kA.as<uint64_t>(),
                                               kB.as<uint64_t>(), (int)T, 32, 32 + n_bits, nullptr));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb2, kB.as<uint64_t>(), kA.as<uint64_t>(), vB.as<uint64_t>(),
                                               vA.as<uint64_t>(), (int)T, 0, 64, nullptr));
    SIG_ALLOC(tmp, std::max<size_t>(std::max(tb1, tb2), 256)); /* never null: a null buffer means "size query" */
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb1, vA.as<uint64_t>(), vB.as<uint64_t>(), kA.as<uint64_t>(),
                                               kB.as<uint64_t>(), (int)T, 32, 32 + n_bits, nullptr));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp.p, tb2, kB.as<uint64_t>(), kA.as<uint64_t>(), vB.as<uint64_t>(),
                                               vA.as<uint64_t>(), (int)T, 0, 64, nullptr));
    if ((rc = R.clock.mark(kOrder)))
        return rc;

    /* sets: heads -> starts (kB / vB are scratch from here) */
    uint8_t *head = vB.as<uint8_t>();        /* T bytes of T * 8 */
    uint32_t *starts = kB.as<uint32_t>();    /* n_sets + 1 <= T + 1 words of 2 * T */
    unsigned long long *d_nsel = R.n_sf();   /* borrowed until the popcount */
    hipLaunchKernelGGL(sig_heads_kernel, dim3((uint32_t)((T + 255) / 256)), dim3(256), 0, nullptr,
                       kA.as<uint64_t>(), (uint32_t)T, head);
    hipcub::CountingInputIterator<uint32_t> ids(0);
    size_t tb = 0;
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, tb, ids, head, starts, d_nsel, (int)T, nullptr));
    SIG_ALLOC(tmp, tb);
    HIP_TRY(hipcub::DeviceSelect::Flagged(tmp.p, tb, ids, head, starts, d_nsel, (int)T, nullptr));
    unsigned long long n_sets = 0;
    HIP_TRY(hipMemcpy(&n_sets, d_nsel, 8, hipMemcpyDeviceToHost));
    if (n_sets == 0 || n_sets > T)
        return fail(KGX_EDEVICE, "signature selection: bad set count");
    const uint32_t t32 = (uint32_t)T;
    HIP_TRY(hipMemcpy(starts + n_sets, &t32, 4, hipMemcpyHostToDevice)); /* T == 1: word 1 of kB's 2 */
    HIP_TRY(hipMemset(d_nsel, 0, 8));
    st.n_sets += n_sets;

    /* segment */
    SIG_ALLOC(R.best, n_sets * 4);
    SIG_ALLOC(R.nbest, n_sets * 4);
    SIG_ALLOC(R.keep, n_sets);
    /* a listed set holds more than kSmallSet tuples */
    const uint64_t list_cap = T / (kSmallSet + 1) + 1, block_cap = T / (kWaveSet + 1) + 1;
    SIG_ALLOC(R.lists, (list_cap + block_cap) * 4);
    const SetOut so{R.best.as<int32_t>(), R.nbest.as<uint32_t>(), R.keep.as<uint8_t>()};
    uint32_t *wave_list = R.lists.as<uint32_t>(), *block_list = wave_list + list_cap;
    uint32_t *bitmap = R.bitmap.as<uint32_t>();
    hipLaunchKernelGGL(sig_small_kernel, sig_grid(n_sets), dim3(256), 0, nullptr, starts, (uint32_t)n_sets,
                       vA.as<uint64_t>(), R.fn.as<int32_t>(), so, bitmap, wave_list, block_list, R.n_lists());
    hipLaunchKernelGGL(sig_wave_kernel, sig_grid(list_cap, 4, 2048), dim3(256), 0, nullptr, starts, wave_list,
                       R.n_lists(), vA.as<uint64_t>(), R.fn.as<int32_t>(), so, bitmap);
    hipLaunchKernelGGL(sig_block_kernel, sig_grid(block_cap, 1, 2048), dim3(256), 0, nullptr, starts, block_list,
                       R.n_lists() + 1, vA.as<uint64_t>(), R.fn.as<int32_t>(), so, bitmap);
    HIP_TRY(hipGetLastError());
    if ((rc = R.clock.mark(kSegment)))
        return rc;

    /* the kept sets in set order and their records; of the only pass with NSF, hence final */
    if (only)
        hipLaunchKernelGGL(sig_popcount_kernel, sig_grid(R.n_words, 256, 1024), dim3(256), 0, nullptr, bitmap,
                           R.n_words, R.n_sf());
    const uint64_t kept_bytes = (n_sets * 4 + 7) & ~7ull; /* the ids, then their count */
    SIG_ALLOC(R.kept, kept_bytes + 8);
    unsigned long long *d_nkept = reinterpret_cast<unsigned long long *>(R.kept.as<uint8_t>() + kept_bytes);
    tb = 0;
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, tb, ids, R.keep.as<uint8_t>(), R.kept.as<uint32_t>(), d_nkept,
                                          (int)n_sets, nullptr));
    SIG_ALLOC(tmp, tb);
    HIP_TRY(hipcub::DeviceSelect::Flagged(tmp.p, tb, ids, R.keep.as<uint8_t>(), R.kept.as<uint32_t>(), d_nkept,
                                          (int)n_sets, nullptr));
    unsigned long long n_kept = 0, nsf = 0;
    HIP_TRY(hipMemcpy(&n_kept, d_nkept, 8, hipMemcpyDeviceToHost));
    if (only)
        HIP_TRY(hipMemcpy(&nsf, R.n_sf(), 8, hipMemcpyDeviceToHost));
    if (n_kept > n_sets)
        return fail(KGX_EDEVICE, "signature selection: bad kept count");
    st.n_kept += n_kept;
    DevBuf recs;
    if (n_kept) {
        SIG_ALLOC(recs, n_kept * sizeof(kgx_sig_record));
        const auto records = only ? sig_records_kernel<true> : sig_records_kernel<false>;
        hipLaunchKernelGGL(records, sig_grid(n_kept), dim3(256), 0, nullptr, R.kept.as<uint32_t>(), (uint32_t)n_kept,
                           starts, kA.as<uint64_t>(), vA.as<uint64_t>(), so, R.nfn.as<uint32_t>(), (float)nsf,
                           recs.as<kgx_sig_record>(), R.n_stor());
        HIP_TRY(hipGetLastError());
    }
    if (only) {
        unsigned long long n_stor = 0;
        HIP_TRY(hipMemcpy(&n_stor, R.n_stor(), 8, hipMemcpyDeviceToHost));
        st.n_storable = n_stor;
        st.n_seqs_with_signature = nsf;
    }
    R.S->chunk.push_back(std::move(recs));
    R.S->passes.push_back(kgx_sig_pass{lo, hi, T, n_sets, n_kept});
    if ((rc = R.clock.mark(kRecords)))
        return rc;
    return R.clock.flush();
}

int sig_select(kgx_sig *S, const char *residues, const uint64_t *seq_offsets, const int32_t *seq_function,
               uint32_t n_seq, const std::vector<uint32_t> &n_fn, uint64_t cap, uint32_t max_len, uint64_t budget)
{
    const uint64_t base = seq_offsets[0], total = seq_offsets[n_seq] - base;
    kgx_sig_stats &st = S->stats;
    st.n_windows = cap;
    st.num_sigs_rule = builder_num_sigs(0);
    if (cap == 0)
        return KGX_OK;
    SigRun R(S);
    R.total = total;
    R.n_seq = n_seq;
    R.max_len = max_len;
    R.n_words = (n_seq + 31) / 32;
    int rc = R.clock.mark(kUpload);
    if (rc)
        return rc;

    /* upload: residues, offsets from 0, functions, sequences per function */
    SIG_ALLOC(R.res, total);
    SIG_ALLOC(R.off, ((uint64_t)n_seq + 1) * 8);
    SIG_ALLOC(R.fn, (uint64_t)n_seq * 4);
    SIG_ALLOC(R.nfn, std::max<uint64_t>(n_fn.size(), 1) * 4);
    SIG_ALLOC(R.cnt, 4 * 8);
    SIG_ALLOC(R.bitmap, (uint64_t)R.n_words * 4);
    {
        std::vector<uint64_t> off0(n_seq + 1);
        for (uint32_t i = 0; i <= n_seq; i++)
            off0[i] = seq_offsets[i] - base;
        HIP_TRY(hipMemcpy(R.off.p, off0.data(), off0.size() * 8, hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemcpy(R.res.p, residues + base, total, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(R.fn.p, seq_function, (uint64_t)n_seq * 4, hipMemcpyHostToDevice));
    if (!n_fn.empty())
        HIP_TRY(hipMemcpy(R.nfn.p, n_fn.data(), n_fn.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(R.bitmap.p, 0, (uint64_t)R.n_words * 4));
    if (budget == 0) {
        size_t free_bytes = 0, all_bytes = 0;
        HIP_TRY(hipMemGetInfo(&free_bytes, &all_bytes));
        budget = sig_auto_budget(free_bytes, cap);
    }
    if ((rc = R.clock.mark(kUpload)))
        return rc;

    /* within the budget: one pass over every key, nothing counted */
    if (cap <= budget)
        return sig_pass(R, 0, kSigAllKeys, cap, false, true, true);

    /* the passes, planned from counts on the device (timed as emit) */
    std::vector<SigPass> plan;
    SIG_ALLOC(R.bins, kSigBins * 8);
    SigPlanner planner(budget, [&R](uint64_t prefix, int d, uint64_t *counts) { return sig_count(R, prefix, d, counts); });
    if ((rc = planner.plan(&plan)))
        return rc == KGX_ERANGE && !planner.error().empty() ? fail(rc, planner.error()) : rc;
    if (plan.empty()) { /* no tuple anywhere */
        if ((rc = R.clock.mark(kEmit)))
            return rc;
        return R.clock.flush();
    }
    uint64_t largest = 0;
    for (const SigPass &p : plan)
        largest = std::max(largest, p.n_tuples);
    SIG_ALLOC(R.kA, largest * 8);
    SIG_ALLOC(R.vA, largest * 8);
    SIG_ALLOC(R.kB, largest * 8);
    SIG_ALLOC(R.vB, largest * 8);
    const bool only = plan.size() == 1;
    for (size_t i = 0; i < plan.size(); i++)
        if ((rc = sig_pass(R, plan[i].lo_key, plan[i].hi_key, plan[i].n_tuples, true, i + 1 == plan.size(), only)))
            return rc;
    if (only)
        return KGX_OK;

    /* NSF and KS are whole: the weights */
    hipLaunchKernelGGL(sig_popcount_kernel, sig_grid(R.n_words, 256, 1024), dim3(256), 0, nullptr,
                       R.bitmap.as<uint32_t>(), R.n_words, R.n_sf());
    HIP_TRY(hipGetLastError());
    unsigned long long nsf = 0, n_stor = 0;
    HIP_TRY(hipMemcpy(&nsf, R.n_sf(), 8, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < S->chunk.size(); i++)
        if (S->passes[i].n_kept)
            hipLaunchKernelGGL(sig_weights_kernel, sig_grid(S->passes[i].n_kept), dim3(256), 0, nullptr,
                               S->chunk[i].as<kgx_sig_record>(), S->passes[i].n_kept, R.nfn.as<uint32_t>(),
                               (float)nsf, (float)st.n_kept, R.n_stor());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&n_stor, R.n_stor(), 8, hipMemcpyDeviceToHost));
    st.n_storable = n_stor;
    st.n_seqs_with_signature = nsf;
    if ((rc = R.clock.mark(kRecords)))
        return rc;
    return R.clock.flush();
}

}  // namespace

extern "C" {

int kgx_sig_select(int device, const char *residues, const uint64_t *seq_offsets, const int32_t *seq_function,
                   uint32_t n_seq, uint32_t n_functions, kgx_sig **out)
{
    return kgx_sig_select_passes(device, residues, seq_offsets, seq_function, n_seq, n_functions, 0, out);
}

int kgx_sig_select_passes(int device, const char *residues, const uint64_t *seq_offsets, const int32_t *seq_function,
                          uint32_t n_seq, uint32_t n_functions, uint64_t max_pass_tuples, kgx_sig **out)
{
    if (!out || !seq_offsets || (n_seq && !seq_function))
        return fail(KGX_EINVAL, "null argument");
    *out = nullptr;
    if (max_pass_tuples > kSigMaxPassTuples) /* hipCUB counts items in an int */
        return fail(KGX_EINVAL, "max_pass_tuples = " + std::to_string(max_pass_tuples) + " is above 2^31-1");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
        return fail(KGX_EDEVICE, "no such HIP device " + std::to_string(device));
    if (!is_gfx950(device))
        return fail(KGX_EDEVICE, "device " + std::to_string(device) + " is not gfx950");
    /* NF and the window count; sequences without a kept function (< 0) give nothing */
    std::vector<uint32_t> n_fn(n_functions, 0);
    uint64_t cap = 0, max_len = 0;
    for (uint32_t i = 0; i < n_seq; i++) {
        if (seq_offsets[i + 1] < seq_offsets[i])
            return fail(KGX_EINVAL, "seq_offsets not monotone");
        const uint64_t len = seq_offsets[i + 1] - seq_offsets[i];
        if (len > 0x7FFFFFFFull)
            return fail(KGX_ERANGE, "sequence " + std::to_string(i) + " is longer than 2^31-1 residues");
        const int32_t f = seq_function[i];
        if (f < 0)
            continue;
        if ((uint32_t)f >= n_functions)
            return fail(KGX_ERANGE, "seq_function[" + std::to_string(i) + "] = " + std::to_string(f) +
                                        " is not below n_functions = " + std::to_string(n_functions));
        n_fn[f]++;
        cap += len >= 8 ? len - 7 : 0;
        max_len = std::max(max_len, len);
    }
    if (cap && !residues)
        return fail(KGX_EINVAL, "null residues");
    HIP_TRY(hipSetDevice(device));
    kgx_sig *S = new kgx_sig;
    S->device = device;
    const int rc = sig_select(S, residues, seq_offsets, seq_function, n_seq, n_fn, cap, (uint32_t)max_len,
                              max_pass_tuples);
    if (rc) {
        delete S;
        return rc;
    }
    S->stats.num_sigs_rule = builder_num_sigs(S->stats.n_kept);
    *out = S;
    return KGX_OK;
}

int kgx_sig_pass_count(const kgx_sig *s, uint32_t *n)
{
    if (!s || !n)
        return fail(KGX_EINVAL, "null argument");
    *n = (uint32_t)s->passes.size();
    return KGX_OK;
}

int kgx_sig_pass_get(const kgx_sig *s, uint32_t i, kgx_sig_pass *out)
{
    if (!s || !out)
        return fail(KGX_EINVAL, "null argument");
    if (i >= s->passes.size())
        return fail(KGX_ERANGE, "pass " + std::to_string(i) + " of " + std::to_string(s->passes.size()));
    *out = s->passes[i];
    return KGX_OK;
}

int kgx_sig_stats_get(const kgx_sig *s, kgx_sig_stats *out)
{
    if (!s || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = s->stats;
    return KGX_OK;
}

int kgx_sig_stage_ms(const kgx_sig *s, float *ms)
{
    if (!s || !ms)
        return fail(KGX_EINVAL, "null argument");
    std::copy(s->stage_ms, s->stage_ms + kSigStages, ms);
    return KGX_OK;
}

int kgx_sig_records(kgx_sig *s, const kgx_sig_record **recs, uint64_t *n)
{
    if (!s || !recs || !n)
        return fail(KGX_EINVAL, "null argument");
    if (!s->host_valid) {
        HIP_TRY(hipSetDevice(s->device));
        s->host.resize(s->stats.n_kept);
        uint64_t at = 0;
        for (size_t i = 0; i < s->chunk.size(); at += s->passes[i++].n_kept)
            if (s->passes[i].n_kept)
                HIP_TRY(hipMemcpy(s->host.data() + at, s->chunk[i].p, s->passes[i].n_kept * sizeof(kgx_sig_record),
                                  hipMemcpyDeviceToHost));
        s->host_valid = true;
    }
    *recs = s->host.data();
    *n = s->host.size();
    return KGX_OK;
}

int kgx_sig_image(kgx_sig *s, uint64_t num_sigs, kgx_image **out, uint64_t *n_stored)
{
    if (!s || !out)
        return fail(KGX_EINVAL, "null argument");
    if (num_sigs == 0)
        num_sigs = s->stats.num_sigs_rule;
    if (num_sigs == 0)
        return fail(KGX_ERANGE, "Cannot find prime for " + std::to_string(s->stats.n_kept));
    /* kguts.cc:209-213, as kgx_image_build */
    if (s->stats.n_storable >= num_sigs / 2)
        return fail(KGX_EFULL, "Your Kmer hash is half-full (kguts.cc:209-213)");
    HIP_TRY(hipSetDevice(s->device));
    const uint64_t n = s->stats.n_kept, m = std::max<uint64_t>(n, 1);
    DevBuf keys, fi, otu, avg, wt;
    SIG_ALLOC(keys, m * 8);
    SIG_ALLOC(fi, m * 4);
    SIG_ALLOC(otu, m * 4);
    SIG_ALLOC(avg, m * 2);
    SIG_ALLOC(wt, m * 4);
    uint64_t at = 0;
    for (size_t i = 0; i < s->chunk.size(); at += s->passes[i++].n_kept) {
        const uint64_t c = s->passes[i].n_kept; /* a pass's: fewer than 2^31 */
        if (!c)
            continue;
        hipLaunchKernelGGL(sig_entries_kernel, dim3((uint32_t)((c + 255) / 256)), dim3(256), 0, nullptr,
                           s->chunk[i].as<kgx_sig_record>(), c, at, keys.as<uint64_t>(), fi.as<int32_t>(),
                           otu.as<int32_t>(), avg.as<uint16_t>(), wt.as<float>());
        HIP_TRY(hipGetLastError());
    }
    return image_from_device_entries(s->device, num_sigs, keys.as<uint64_t>(), fi.as<int32_t>(), otu.as<int32_t>(),
                                     avg.as<uint16_t>(), wt.as<float>(), n, out, n_stored);
}

int kgx_sig_destroy(kgx_sig *s)
{
    if (!s)
        return KGX_OK;
    (void)hipSetDevice(s->device);
    delete s;
    return KGX_OK;
}

} /* extern "C" */
