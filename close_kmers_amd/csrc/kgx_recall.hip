/*
 * kgx_recall.hip -- build_signature_kmers.cc's recall / validation pass on the
 * device: labelled proteins go back through an image and
 * their best calls are compared with their labels.
 *
 * The reference (--recall-output, :900-978 and :1386-1433; --validation-folder,
 * :984-1026 and :1435-1491) calls process_aa_seq + find_best_call per protein
 * and compares the called function's string with the definitions'.  Here the
 * corpus runs in pieces of whole sequences through the context's own pass
 * (plan, probe, score, find_best_call: kgx_run_device with KGX_WANT_BEST);
 * after each piece one kernel reads the piece's kgx_best_call array and the
 * labels and leaves in HBM
 *   - the best call, appended to the run's array (24 B per sequence: the only
 *     per-sequence record that reaches the host),
 *   - the 3 x 4 cells label class x call class,
 *   - {labelled, correct, called} per function,
 *   - one flag byte per sequence: "changed" (the reference's New rows),
 *   - one 64-bit word per sequence: label << 32 | called for a kept / mismatch
 *     sequence, all ones otherwise.
 * After the last piece the flags are compacted into the ascending changed list
 * (hipCUB DeviceSelect::Flagged over a counting iterator, as kgx_sig.hip
 * compacts its kept sets) and the words are sorted and run-length encoded into
 * the confusion pairs; the all-ones run, which sorts last, is dropped.
 *
 * Same-address atomics (§8.8): one function can hold a large share of a corpus,
 * so a wave takes its distinct function indices one ballot at a time (as the
 * rollup takes its ids, kgx_tables.hip) and one lane adds the group's
 * population count; the cells are twelve ballots per wave, summed over the
 * workgroup's four waves in LDS, and a workgroup adds each non-zero cell once.
 */
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "kgx.h"
#include "kgx_device.h"
#include "kgx_rt.h"

namespace kgx {

constexpr uint64_t kRecallPiece = 1ull << 25;  /* piece_residues 0 */
constexpr uint64_t kNoPair = ~0ull;
constexpr uint32_t kCells = 12;

/* call class of a best call against a label: 0 match, 1 mismatch, 2 ambiguous, 3 none */
__host__ __device__ inline uint32_t recall_call_class(int32_t kind, int32_t fi0, int32_t label)
{
    return kind == 1 ? (fi0 == label ? 0u : 1u) : kind == 2 ? 2u : 3u;
}
/* label class: 0 kept, 1 other, 2 none */
__host__ __device__ inline uint32_t recall_label_class(int32_t label)
{
    return label >= 0 ? 0u : label == KGX_LABEL_OTHER ? 1u : 2u;
}

/* `mine` lanes hold a function index below n_functions: each distinct one
 * gets one add of its lanes' number to its counter in `first`, and one of
 * those among them with `extra` set to its counter in `second` (counters are
 * three words apart: kgx_recall_function) */
__device__ __forceinline__ void recall_add_grouped(bool mine, uint32_t idx, uint32_t *first, bool extra, uint32_t *second)
{
    uint64_t rem = __ballot(mine);
    while (rem) {
        const uint32_t ld = lowbit(rem);
        const uint32_t v = rl32(idx, ld);
        const bool in = mine && idx == v;
        const uint64_t grp = __ballot(in);
        const uint64_t ext = __ballot(in && extra);
        rem &= ~grp;
        if (lane_id() == ld) {
            atomicAdd(first + 3ull * v, (uint32_t)__popcll(grp));
            if (ext)
                atomicAdd(second + 3ull * v, (uint32_t)__popcll(ext));
        }
    }
}

/* One thread per sequence of a piece: best[0, n) are the piece's calls,
 * label / best_all / changed / pair are the run's arrays at the piece's first
 * sequence.  fn: n_functions x {labelled, correct, called}.  A call naming a
 * function that is not below n_functions sets *status and touches no counter
 * of that function. */
__global__ __launch_bounds__(256) void recall_tally_kernel(const kgx_best_call *__restrict__ best, uint32_t n,
                                                           const int32_t *__restrict__ label, uint32_t n_functions,
                                                           kgx_best_call *__restrict__ best_all,
                                                           uint8_t *__restrict__ changed, uint64_t *__restrict__ pair,
                                                           uint32_t *fn, unsigned long long *cell, uint32_t *status)
{
    __shared__ uint32_t s_cell[kCells];
    if (threadIdx.x < kCells)
        s_cell[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < n;
    kgx_best_call b;
    b.kind = 0;
    b.fi0 = b.fi1 = -1;
    b.score = b.weighted_score = b.score_offset = 0.0f;
    int32_t lab = KGX_LABEL_NONE;
    if (valid) {
        b = best[i];
        lab = label[i];
        best_all[i] = b;
    }
    /* the functions a call names: fi0 of kinds 1 to 3, fi1 of kinds 2 and 3 (-1: none) */
    const bool named0 = b.kind != 0 && b.fi0 != -1, named1 = b.kind != 0 && b.kind != 1 && b.fi1 != -1;
    const bool bad = (named0 && (uint32_t)b.fi0 >= n_functions) || (named1 && (uint32_t)b.fi1 >= n_functions) ||
                     (b.kind == 1 && !named0);
    if (bad)
        atomicOr(status, 1u);
    const uint32_t cc = recall_call_class(b.kind, b.fi0, lab), lc = recall_label_class(lab);
    if (valid) {
        changed[i] = cc == 3u ? lab != KGX_LABEL_NONE : cc != 0u;
        pair[i] = (lc == 0u && cc == 1u) ? ((uint64_t)(uint32_t)lab << 32 | (uint32_t)b.fi0) : kNoPair;
    }
    /* cells: a ballot per cell, the wave's counts into LDS, the workgroup's into HBM */
    const uint32_t mycell = lc * 4u + cc;
    for (uint32_t k = 0; k < kCells; k++) {
        const uint64_t m = __ballot(valid && mycell == k);
        if (m && lane_id() == 0)
            atomicAdd(&s_cell[k], (uint32_t)__popcll(m));
    }
    /* per function: labelled and correct share the label, called has fi0 */
    recall_add_grouped(valid && lc == 0u && (uint32_t)lab < n_functions, (uint32_t)lab, fn, cc == 0u, fn + 1);
    recall_add_grouped(valid && b.kind == 1 && !bad, (uint32_t)b.fi0, fn + 2, false, fn + 2);
    __syncthreads();
    if (threadIdx.x < kCells && s_cell[threadIdx.x])
        atomicAdd(cell + threadIdx.x, (unsigned long long)s_cell[threadIdx.x]);
}

}  // namespace kgx

using namespace kgx;

struct kgx_recall {
    kgx_recall_stats stats{};
    std::vector<kgx_best_call> best;
    std::vector<kgx_recall_function> fn;
    std::vector<uint32_t> changed;
    std::vector<kgx_recall_pair> pairs;
};

namespace {

enum { kUp = 0, kPass, kTally, kDown };

/* the timing events of a run: four marks bound the three stages of a piece */
struct RecallEvents {
    hipEvent_t e[4] = {};
    ~RecallEvents()
    {
        for (hipEvent_t x : e)
            if (x)
                (void)hipEventDestroy(x);
    }
    int create()
    {
        for (hipEvent_t &x : e)
            HIP_TRY(hipEventCreate(&x));
        return KGX_OK;
    }
    /* the time between marks a and b (both reached) goes to stage s */
    int add(int a, int b, int s, float *ms)
    {
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e[a], e[b]));
        ms[s] += t;
        return KGX_OK;
    }
};

}  // namespace

namespace kgx {

/* as the host batches cut (kgx_host_batch.cpp cut_at_nul): from the residue
 * before the first NUL on, a staged sequence reads 'X' */
static void recall_cut_at_nul(char *b, uint64_t len)
{
    const void *z = len ? std::memchr(b, 0, len) : nullptr;
    if (!z)
        return;
    const uint64_t slen = (uint64_t)((const char *)z - b);
    for (uint64_t i = slen ? slen - 1 : 0; i < len; i++)
        b[i] = 'X';
}

/* A piece's n residues from the caller's (pageable) src into the context's
 * pinned staging and up to its device buffer, on its stream, in slices: the
 * staging threads copy and NUL-scan a slice while the DMA engine moves the
 * one before.  A NUL anywhere is rare: the staged piece is then cut sequence
 * by sequence (off: its m + 1 absolute offsets) and goes up again whole. */
int recall_stage_upload(kgx_ctx *c, const char *src, uint64_t n, const uint64_t *off, uint32_t m)
{
    constexpr uint64_t kSlice = 8ull << 20;
    if (n == 0)
        return KGX_OK;
    char *dst = c->h_res.data();
    const unsigned want_threads = (unsigned)std::max<int64_t>(c->opt.stage_threads, 1);
    if (n >= (1u << 20) && want_threads > 1 && (!c->stage_pool || c->stage_pool->size() != want_threads))
        c->stage_pool.reset(new HostPool(want_threads));
    HostPool *sp = n >= (1u << 20) && want_threads > 1 ? c->stage_pool.get() : nullptr;
    std::atomic<bool> nul{false};
    for (uint64_t a = 0; a < n; a += kSlice) {
        const uint64_t len = std::min(kSlice, n - a);
        const unsigned P = sp ? sp->size() : 1;
        for (unsigned p = 0; p < P; p++) {
            const uint64_t lo = a + len * p / P, hi = a + len * (p + 1) / P;
            auto part = [dst, src, lo, hi, &nul]() -> int {
                std::memcpy(dst + lo, src + lo, hi - lo);
                if (std::memchr(dst + lo, 0, hi - lo))
                    nul.store(true, std::memory_order_relaxed);
                return KGX_OK;
            };
            if (sp)
                sp->submit(part);
            else
                (void)part();
        }
        if (sp)
            (void)sp->wait();
        HIP_TRY(hipMemcpyAsync(c->residues.as<char>() + a, dst + a, len, hipMemcpyHostToDevice, c->stream));
    }
    if (!nul.load())
        return KGX_OK;
    HIP_TRY(hipStreamSynchronize(c->stream)); /* the slices have left the staging buffer */
    for (uint32_t i = 0; i < m; i++)
        recall_cut_at_nul(dst + (off[i] - off[0]), off[i + 1] - off[i]);
    HIP_TRY(hipMemcpyAsync(c->residues.p, dst, n, hipMemcpyHostToDevice, c->stream));
    return KGX_OK;
}

}  // namespace kgx

namespace {

/* the run's device arrays */
struct RecallDev {
    DevBuf label, best, changed, pair, fn, cell, list, keys, runs, counts, tmp;
    /* cell: 12 cells | the selection's count | the runs' count (u64 each); then the status word */
    unsigned long long *cells() const { return cell.as<unsigned long long>(); }
    unsigned long long *n_sel() const { return cells() + kCells; }
    unsigned long long *n_runs() const { return cells() + kCells + 1; }
    uint32_t *status() const { return reinterpret_cast<uint32_t *>(cells() + kCells + 2); }
    static constexpr size_t cell_bytes = (kCells + 3) * 8;
};

#define RECALL_ALLOC(buf, bytes)                                                               \
    do {                                                                                       \
        if ((buf).reserve(bytes) != hipSuccess) {                                              \
            (void)hipGetLastError();                                                           \
            return fail(KGX_ENOMEM, "recall: the corpus' tallies do not fit the device (" #buf ")"); \
        }                                                                                      \
    } while (0)

int recall_run(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *off,
               const int32_t *seq_label, uint32_t n_seq, uint32_t n_functions, uint64_t piece_residues, kgx_recall *R)
{
    kgx_recall_stats &st = R->stats;
    st.n_seq = n_seq;
    R->fn.assign(n_functions, kgx_recall_function{0, 0, 0});
    if (n_seq == 0)
        return KGX_OK;
    hipStream_t s = c->stream;
    RecallEvents ev;
    int rc = ev.create();
    if (rc)
        return rc;
    RecallDev D;
    const uint64_t n = n_seq, nf = std::max<uint32_t>(n_functions, 1);
    HIP_TRY(hipEventRecord(ev.e[0], s));
    RECALL_ALLOC(D.label, n * 4);
    RECALL_ALLOC(D.best, n * sizeof(kgx_best_call));
    RECALL_ALLOC(D.changed, n);
    RECALL_ALLOC(D.pair, n * 8);
    RECALL_ALLOC(D.fn, nf * sizeof(kgx_recall_function));
    RECALL_ALLOC(D.cell, RecallDev::cell_bytes);
    HIP_TRY(hipMemcpyAsync(D.label.p, seq_label, n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(D.fn.p, 0, nf * sizeof(kgx_recall_function), s));
    HIP_TRY(hipMemsetAsync(D.cell.p, 0, RecallDev::cell_bytes, s));
    HIP_TRY(hipEventRecord(ev.e[1], s));
    HIP_TRY(hipStreamSynchronize(s)); /* seq_label may be pageable: the caller's array is read by now */
    if ((rc = ev.add(0, 1, kUp, st.stage_ms)))
        return rc;

    /* the pieces, one after the other: stage, upload, pass, tally */
    for (uint32_t s0 = 0; s0 < n_seq;) {
        uint32_t s1 = s0 + 1;
        while (s1 < n_seq && off[s1 + 1] - off[s0] <= piece_residues)
            s1++;
        const uint32_t m = s1 - s0;
        const uint64_t r0 = off[s0], n_res = off[s1] - r0;
        if (n_res > (1ull << 40))
            return fail(KGX_ERANGE, "recall: a piece of " + std::to_string(n_res) + " residues");
        HIP_TRY(hipEventRecord(ev.e[0], s));
        HIP_TRY(c->h_res.resize(n_res));
        HIP_TRY(c->h_off_stage.resize(m + 1));
        for (uint32_t i = 0; i <= m; i++)
            c->h_off_stage[i] = off[s0 + i] - r0;
        HIP_TRY(c->residues.reserve(n_res + 16));
        HIP_TRY(c->offsets.reserve((m + 1ull) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(c->offsets.p, c->h_off_stage.data(), (m + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice,
                               s));
        if ((rc = recall_stage_upload(c, residues + r0, n_res, off + s0, m)))
            return rc;
        HIP_TRY(hipEventRecord(ev.e[1], s));
        if ((rc = kgx_run_device(c, params, c->residues.as<uint8_t>(), c->offsets.as<uint64_t>(), m, n_res,
                                 KGX_WANT_BEST, nullptr)))
            return rc;
        if (!c->have_best || !c->best.p)
            return fail(KGX_EDEVICE, "recall: the pass left no best calls");
        HIP_TRY(hipEventRecord(ev.e[2], s));
        hipLaunchKernelGGL(recall_tally_kernel, dim3((m + 255u) / 256u), dim3(256), 0, s, c->best.as<kgx_best_call>(), m,
                           D.label.as<int32_t>() + s0, n_functions, D.best.as<kgx_best_call>() + s0,
                           D.changed.as<uint8_t>() + s0, D.pair.as<uint64_t>() + s0, D.fn.as<uint32_t>(), D.cells(),
                           D.status());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev.e[3], s));
        /* the staging buffers and the context's arrays are the next piece's too */
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = ev.add(0, 1, kUp, st.stage_ms)) || (rc = ev.add(1, 2, kPass, st.stage_ms)) ||
            (rc = ev.add(2, 3, kTally, st.stage_ms)))
            return rc;
        st.n_pieces++;
        s0 = s1;
    }

    /* a call outside the function index: nothing was counted for it, and nothing is returned */
    uint32_t status = 0;
    HIP_TRY(hipMemcpyAsync(&status, D.status(), 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status)
        return fail(KGX_ERANGE, "recall: the image calls a function that is not below n_functions = " +
                                    std::to_string(n_functions));

    /* the changed list and the confusion pairs (timed as tally) */
    HIP_TRY(hipEventRecord(ev.e[0], s));
    RECALL_ALLOC(D.list, n * 4);
    RECALL_ALLOC(D.keys, n * 8);
    RECALL_ALLOC(D.runs, n * 8);
    RECALL_ALLOC(D.counts, n * 4);
    hipcub::CountingInputIterator<uint32_t> ids(0);
    size_t tb1 = 0, tb2 = 0, tb3 = 0;
    HIP_TRY(hipcub::DeviceSelect::Flagged(nullptr, tb1, ids, D.changed.as<uint8_t>(), D.list.as<uint32_t>(), D.n_sel(),
                                          (int)n, s));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(nullptr, tb2, D.pair.as<uint64_t>(), D.keys.as<uint64_t>(), (int)n, 0, 64,
                                              s));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(nullptr, tb3, D.keys.as<uint64_t>(), D.runs.as<uint64_t>(),
                                                  D.counts.as<uint32_t>(), D.n_runs(), (int)n, s));
    RECALL_ALLOC(D.tmp, std::max<size_t>(std::max(tb1, std::max(tb2, tb3)), 256)); /* never null: that asks for the size */
    HIP_TRY(hipcub::DeviceSelect::Flagged(D.tmp.p, tb1, ids, D.changed.as<uint8_t>(), D.list.as<uint32_t>(), D.n_sel(),
                                          (int)n, s));
    HIP_TRY(hipcub::DeviceRadixSort::SortKeys(D.tmp.p, tb2, D.pair.as<uint64_t>(), D.keys.as<uint64_t>(), (int)n, 0, 64,
                                              s));
    HIP_TRY(hipcub::DeviceRunLengthEncode::Encode(D.tmp.p, tb3, D.keys.as<uint64_t>(), D.runs.as<uint64_t>(),
                                                  D.counts.as<uint32_t>(), D.n_runs(), (int)n, s));
    HIP_TRY(hipEventRecord(ev.e[1], s));

    /* download: the counters first (they size the two lists), then the arrays */
    unsigned long long h_cell[kCells + 2] = {};
    HIP_TRY(hipMemcpyAsync(h_cell, D.cells(), sizeof(h_cell), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t n_changed = h_cell[kCells], n_runs = h_cell[kCells + 1];
    if (n_changed > n || n_runs > n || n_runs == 0)
        return fail(KGX_EDEVICE, "recall: bad list sizes");
    for (uint32_t k = 0; k < kCells; k++)
        st.cell[k / 4][k % 4] = h_cell[k];
    R->best.resize(n);
    R->changed.resize(n_changed);
    std::vector<uint64_t> keys(n_runs);
    std::vector<uint32_t> counts(n_runs);
    HIP_TRY(hipMemcpyAsync(R->best.data(), D.best.p, n * sizeof(kgx_best_call), hipMemcpyDeviceToHost, s));
    if (n_functions)
        HIP_TRY(hipMemcpyAsync(R->fn.data(), D.fn.p, (uint64_t)n_functions * sizeof(kgx_recall_function),
                               hipMemcpyDeviceToHost, s));
    if (n_changed)
        HIP_TRY(hipMemcpyAsync(R->changed.data(), D.list.p, n_changed * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(keys.data(), D.runs.p, n_runs * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(counts.data(), D.counts.p, n_runs * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = ev.add(0, 1, kTally, st.stage_ms)) || (rc = ev.add(1, 2, kDown, st.stage_ms)))
        return rc;
    /* the sequences without a pair sort last, as one run */
    const uint64_t n_pairs = keys[n_runs - 1] == kNoPair ? n_runs - 1 : n_runs;
    R->pairs.resize(n_pairs);
    for (uint64_t i = 0; i < n_pairs; i++)
        R->pairs[i] = kgx_recall_pair{(int32_t)(keys[i] >> 32), (int32_t)(uint32_t)keys[i], counts[i]};
    st.n_changed = n_changed;
    st.n_confusions = n_pairs;
    return KGX_OK;
}

}  // namespace

extern "C" {

int kgx_recall_run(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                   const int32_t *seq_label, uint32_t n_seq, uint32_t n_functions, uint64_t piece_residues,
                   kgx_recall **out)
{
    if (!out)
        return fail(KGX_EINVAL, "null argument");
    *out = nullptr;
    if (!c || !seq_offsets || (n_seq && !seq_label))
        return fail(KGX_EINVAL, "null argument");
    if (n_seq > 0x7FFFFFFFu) /* hipCUB counts items in an int */
        return fail(KGX_ERANGE, "recall: more than 2^31-1 sequences");
    for (uint32_t i = 0; i < n_seq; i++) {
        if (seq_offsets[i + 1] < seq_offsets[i])
            return fail(KGX_EINVAL, "seq_offsets not monotone");
        const int32_t l = seq_label[i];
        if (l < KGX_LABEL_NONE || (l >= 0 && (uint32_t)l >= n_functions))
            return fail(KGX_EINVAL, "seq_label[" + std::to_string(i) + "] = " + std::to_string(l) +
                                        " is neither a label class nor below n_functions = " +
                                        std::to_string(n_functions));
    }
    if (n_seq && seq_offsets[n_seq] > seq_offsets[0] && !residues)
        return fail(KGX_EINVAL, "null residues");
    if (!is_gfx950(c->img->device))
        return fail(KGX_EDEVICE, "device " + std::to_string(c->img->device) + " is not gfx950");
    HIP_TRY(hipSetDevice(c->img->device));
    kgx_params p;
    if (params)
        p = *params;
    else
        kgx_params_default(&p);
    kgx_recall *R = new kgx_recall;
    const int rc = recall_run(c, &p, residues, seq_offsets, seq_label, n_seq, n_functions,
                              piece_residues ? piece_residues : kRecallPiece, R);
    if (rc) {
        (void)hipStreamSynchronize(c->stream); /* nothing of this call is in flight when its arrays go */
        delete R;
        return rc;
    }
    *out = R;
    return KGX_OK;
}

int kgx_recall_stats_get(const kgx_recall *r, kgx_recall_stats *out)
{
    if (!r || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = r->stats;
    return KGX_OK;
}

int kgx_recall_best(const kgx_recall *r, const kgx_best_call **best, uint64_t *n)
{
    if (!r || !best || !n)
        return fail(KGX_EINVAL, "null argument");
    *best = r->best.data();
    *n = r->best.size();
    return KGX_OK;
}

int kgx_recall_functions(const kgx_recall *r, const kgx_recall_function **fn, uint32_t *n)
{
    if (!r || !fn || !n)
        return fail(KGX_EINVAL, "null argument");
    *fn = r->fn.data();
    *n = (uint32_t)r->fn.size();
    return KGX_OK;
}

int kgx_recall_changed(const kgx_recall *r, const uint32_t **seq, uint64_t *n)
{
    if (!r || !seq || !n)
        return fail(KGX_EINVAL, "null argument");
    *seq = r->changed.data();
    *n = r->changed.size();
    return KGX_OK;
}

int kgx_recall_confusions(const kgx_recall *r, const kgx_recall_pair **pairs, uint64_t *n)
{
    if (!r || !pairs || !n)
        return fail(KGX_EINVAL, "null argument");
    *pairs = r->pairs.data();
    *n = r->pairs.size();
    return KGX_OK;
}

int kgx_recall_destroy(kgx_recall *r)
{
    delete r;
    return KGX_OK;
}

} /* extern "C" */
