/*
 * kgx_host_batch.cpp -- host-buffer batches of the C ABI (include/kgx.h):
 * kgx_process_batch and its schedules (streamed and exact chunks, one pass,
 * small, fused), their staging, the compact records' expansion on the host,
 * and kgx_process_batch_compact / kgx_compact_expand.  Images, contexts and
 * the device stages are in kgx_runtime.cpp.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kgx_rt.h"

using namespace kgx;

extern "C" {

/* ---- host-buffer batch ---------------------------------------------------- */

namespace {

/* a sequence is cut at its first NUL (strlen bound of gather_hits,
 * kguts.cc:792): the NUL's predecessor and everything after become 'X', which
 * kills exactly the windows the reference never visits */
void cut_at_nul(char *b, uint64_t len)
{
    const void *z = len ? std::memchr(b, 0, len) : nullptr;
    if (z) {
        const uint64_t slen = (uint64_t)((const char *)z - b);
        for (uint64_t i = slen ? slen - 1 : 0; i < len; i++)
            b[i] = 'X';
    }
}

/* the n + 1 chunk-relative offsets of sequences [s0, s1) */
void stage_offsets_into(uint64_t *off, const uint64_t *seq_offsets, uint32_t s0, uint32_t s1)
{
    const uint32_t n = s1 - s0;
    const uint64_t r0 = n ? seq_offsets[s0] : 0;
    for (uint32_t i = 0; i <= n; i++)
        off[i] = n ? seq_offsets[s0 + i] - r0 : 0;
}

/* sequences [s0, s1) of a host batch -> pinned staging at dst (residues) and
 * off (the n + 1 chunk-relative offsets); host work only, large ranges copied
 * and NUL-scanned in parts on the stage pool sp */
void stage_copy_into(char *dst, uint64_t *off, const char *residues, const uint64_t *seq_offsets, uint32_t s0,
                     uint32_t s1, HostPool *sp)
{
    const uint32_t n = s1 - s0;
    const uint64_t r0 = n ? seq_offsets[s0] : 0;
    const uint64_t n_res = n ? seq_offsets[s1] - r0 : 0;
    bool has_nul = false;
    if (sp && n_res >= (1u << 20)) {
        const unsigned P = sp->size();
        std::atomic<bool> nul{false};
        const char *src = residues + r0;
        for (unsigned p = 0; p < P; p++) {
            const uint64_t a = n_res * p / P, b = n_res * (p + 1) / P;
            sp->submit([dst, src, a, b, &nul]() -> int {
                std::memcpy(dst + a, src + a, b - a);
                if (std::memchr(dst + a, 0, b - a))
                    nul.store(true, std::memory_order_relaxed);
                return KGX_OK;
            });
        }
        (void)sp->wait();
        has_nul = nul.load();
    } else if (n_res) {
        std::memcpy(dst, residues + r0, n_res);
        /* one scan of the whole range first: NUL bytes are rare */
        has_nul = std::memchr(dst, 0, n_res) != nullptr;
    }
    if (has_nul)
        for (uint32_t s = s0; s < s1; s++)
            cut_at_nul(dst + (seq_offsets[s] - r0), seq_offsets[s + 1] - seq_offsets[s]);
    for (uint32_t i = 0; i <= n; i++)
        off[i] = n ? seq_offsets[s0 + i] - r0 : 0;
}

/* sequences [s0, s1) of a host batch -> x's pinned staging */
int stage_host_copy(kgx_ctx *x, const char *residues, const uint64_t *seq_offsets, uint32_t s0, uint32_t s1,
                    HostPool *sp = nullptr)
{
    const uint32_t n = s1 - s0;
    HIP_TRY(x->h_res.resize(n ? seq_offsets[s1] - seq_offsets[s0] : 0));
    HIP_TRY(x->h_off_stage.resize(n + 1));
    stage_copy_into(x->h_res.data(), x->h_off_stage.data(), residues, seq_offsets, s0, s1, sp);
    return KGX_OK;
}

/* the context's staging threads (option stage_threads; null with 1),
 * recreated when the option changed */
HostPool *ensure_stage_pool(kgx_ctx *c)
{
    if (c->opt.stage_threads <= 1)
        return nullptr;
    if (!c->stage_pool || c->stage_pool->size() != (unsigned)c->opt.stage_threads)
        c->stage_pool.reset(new HostPool((unsigned)c->opt.stage_threads));
    return c->stage_pool.get();
}

/* x's staged sequences -> HBM (async on x's stream) */
int stage_upload(kgx_ctx *x)
{
    const uint64_t n_res = x->h_res.size(), n1 = x->h_off_stage.size();
    HIP_TRY(x->residues.reserve(n_res + 16));
    HIP_TRY(x->offsets.reserve(n1 * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(x->offsets.p, x->h_off_stage.data(), n1 * sizeof(uint64_t), hipMemcpyHostToDevice,
                           x->stream));
    if (n_res)
        HIP_TRY(hipMemcpyAsync(x->residues.p, x->h_res.data(), n_res, hipMemcpyHostToDevice, x->stream));
    return KGX_OK;
}

int stage_host_seqs(kgx_ctx *x, const char *residues, const uint64_t *seq_offsets, uint32_t s0, uint32_t s1)
{
    int rc = stage_host_copy(x, residues, seq_offsets, s0, s1);
    return rc ? rc : stage_upload(x);
}

/* one staged chunk on x: H2D, plan/probe/score, counts + window total -> host */
int enqueue_chunk(kgx_ctx *x, const kgx_params *params, uint32_t want, hipEvent_t counts_done)
{
    int rc = stage_upload(x);
    if (rc)
        return rc;
    const uint32_t n = (uint32_t)x->h_off_stage.size() - 1;
    const uint64_t n_res = x->h_res.size();
    if ((rc = kgx_run_device(x, params, x->residues.as<uint8_t>(), x->offsets.as<uint64_t>(), n, n_res, want,
                             nullptr)))
        return rc;
    HIP_TRY(x->h_hcount.resize(n + 1));
    HIP_TRY(x->h_ccount.resize(n + 1));
    HIP_TRY(x->h_ocount.resize(n + 1));
    HIP_TRY(x->h_nwin.resize(1));
    if (n) {
        HIP_TRY(hipMemcpyAsync(x->h_hcount.data(), x->hit_count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               x->stream));
        HIP_TRY(hipMemcpyAsync(x->h_ccount.data(), x->call_count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               x->stream));
        if (want & KGX_WANT_OTU)
            HIP_TRY(hipMemcpyAsync(x->h_ocount.data(), x->otu_count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   x->stream));
    }
    HIP_TRY(hipMemcpyAsync(x->h_nwin.data(), x->wbase.as<uint64_t>() + n, sizeof(uint64_t),
                           hipMemcpyDeviceToHost, x->stream));
    HIP_TRY(hipEventRecord(counts_done, x->stream));
    return KGX_OK;
}

/* residue byte -> code, to_amino_acid_off (kguts.cc:273-339): the 20
 * standard upper-case residues in alphabetical order, anything else 20 */
struct ResidueCodes {
    uint8_t code[256];
    ResidueCodes()
    {
        std::memset(code, 20, sizeof(code));
        const char *aa = "ACDEFGHIKLMNPQRSTVWY";
        for (int i = 0; i < 20; i++)
            code[(uint8_t)aa[i]] = (uint8_t)i;
    }
};
const ResidueCodes kResidueCodes;

/* the 8-mer key of the window at p (encoded_kmer, kguts.cc:438-455) */
inline uint64_t window_key(const uint8_t *p)
{
    const uint8_t *t = kResidueCodes.code;
    const uint32_t ka = ((t[p[0]] * 20u + t[p[1]]) * 20u + t[p[2]]) * 20u + t[p[3]];
    const uint32_t kb = ((t[p[4]] * 20u + t[p[5]]) * 20u + t[p[6]]) * 20u + t[p[7]];
    return (uint64_t)ka * 160000u + kb;
}

}  // namespace

extern "C++" {
namespace kgx {

/* Sequences [a, b) of a compact chunk: table records (dense, CSR order) +
 * the chunk's hit mask -> kgx_hit, position = the hit's mask bit minus the
 * sequence's first window (what gather_kernel computes on the device).
 * 3-word records: the 12-byte form without the key (gather_kernel's hits12),
 * the key re-encoded from the window's residues; 4 words: the 16-byte table
 * records. */

template <bool R12>
static int expand_chunk_t(const kgx_hit_chunk &ch, const uint64_t *hoff, const char *residues,
                          const uint64_t *seq_offsets, uint32_t a, uint32_t b, kgx_hit *out, uint64_t out_base,
                          uint32_t seq_base, bool nt)
{
    const uint64_t *mask = ch.mask;
    for (uint32_t s = a; s < b; s++) {
        uint64_t j = hoff[s];
        const uint64_t j1 = hoff[s + 1];
        if (j == j1)
            continue;
        const uint64_t w0 = ch.window_start[s - ch.seq_begin], w1 = w0 + windows_of(seq_offsets[s + 1] - seq_offsets[s]);
        if (w1 == w0)
            return fail(KGX_EDEVICE, "compact hits: hits for a sequence without windows (" + std::to_string(s) + ")");
        const uint8_t *seq = reinterpret_cast<const uint8_t *>(residues + seq_offsets[s]);
        for (uint64_t g = w0 >> 6; g <= (w1 - 1) >> 6; g++) {
            uint64_t bits = mask[g];
            if (g == w0 >> 6)
                bits &= ~0ull << (w0 & 63);
            if (g == (w1 - 1) >> 6 && (w1 & 63))
                bits &= ~(~0ull << (w1 & 63));
            if (j + (uint64_t)__builtin_popcountll(bits) > j1)
                return fail(KGX_EDEVICE, "compact hits: more mask bits than hits for sequence " + std::to_string(s));
            for (; bits; bits &= bits - 1, j++) {
                const uint32_t pos = (uint32_t)(64 * g + (uint64_t)__builtin_ctzll(bits) - w0);
                const uint32_t *r = ch.records + (R12 ? 3 : 4) * (j - ch.hit_begin);
                packed_bucket pb;
                uint32_t flags;
                if (R12) {
                    pb.lo = window_key(seq + pos) | (uint64_t)r[2] << 35;
                    pb.hi = (uint64_t)r[1] << 32 | r[0];
                    flags = (r[1] >> 28) & 7u;
                } else {
                    pb.lo = (uint64_t)r[1] << 32 | r[0];
                    pb.hi = (uint64_t)r[3] << 32 | r[2];
                    flags = (r[3] >> 28) & 7u;
                }
                const kgx_sig_kmer e = unpack_bucket(pb);
                kgx_hit o;
                o.which_kmer = e.which_kmer;
                o.otu_index = e.otu_index;
                o.avg_from_end = e.avg_from_end;
                o.flags = (uint16_t)flags;
                o.function_index = e.function_index;
                o.function_wt = e.function_wt;
                o.pos = pos;
                o.seq = s + seq_base;
                kgx_hit *dst = out + (j - out_base);
                if (nt) {
                    /* streaming stores: the 32-B records are written once and
                     * not read back here (no read-for-ownership of the lines) */
                    typedef long long v2i __attribute__((vector_size(16)));
                    v2i q[2];
                    std::memcpy(q, &o, sizeof(o));
                    __builtin_nontemporal_store(q[0], reinterpret_cast<v2i *>(dst));
                    __builtin_nontemporal_store(q[1], reinterpret_cast<v2i *>(dst) + 1);
                } else {
                    *dst = o;
                }
            }
        }
        if (j != j1)
            return fail(KGX_EDEVICE, "compact hits: mask and hit count disagree for sequence " + std::to_string(s));
    }
    if (nt)
        __builtin_ia32_sfence(); /* the streaming stores are visible before the task reports done */
    return KGX_OK;
}

int expand_chunk(const kgx_hit_chunk &ch, const uint64_t *hoff, const char *residues, const uint64_t *seq_offsets,
                 uint32_t a, uint32_t b, kgx_hit *out, uint64_t out_base, uint32_t seq_base, bool nt)
{
    if (ch.record_words == 3)
        return expand_chunk_t<true>(ch, hoff, residues, seq_offsets, a, b, out, out_base, seq_base, nt);
    if (ch.record_words == 4)
        return expand_chunk_t<false>(ch, hoff, residues, seq_offsets, a, b, out, out_base, seq_base, nt);
    return fail(KGX_EINVAL, "compact hits: record_words must be 3 or 4");
}

}  // namespace kgx
}  // extern "C++"

extern "C++" {
namespace kgx {

/* kgx_device_batch_collect's first round trip, enqueued: the plan status,
 * window total and per-sequence counts (and, when nothing needs gathering --
 * the /lookup shape, hits staying on the device -- the best calls) by device
 * stores into the mapped pinned arrays, not by DMA: copies from every stream
 * share the DMA engine in order, so a few KB of counts queued behind other
 * contexts' MB uploads (r5m).  A pool enqueues these right behind each
 * shard's pass, so they do not wait in a shared hardware queue behind a later
 * shard's work (r5s). */
int collect_counts_enqueue(kgx_ctx *c, uint32_t want)
{
    const bool want_calls = (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = (want & KGX_WANT_OTU) != 0;
    const bool need_hits = (want & KGX_WANT_HITS) != 0;
    const bool want_best = (want & KGX_WANT_BEST) != 0;
    const uint32_t n_seq = c->n_seq;
    HIP_TRY(hipSetDevice(c->img->device));
    HIP_TRY(c->h_hcount.resize(n_seq + 1));
    HIP_TRY(c->h_ccount.resize(n_seq + 1));
    HIP_TRY(c->h_ocount.resize(n_seq + 1));
    HIP_TRY(c->h_plan_status.resize(1));
    HIP_TRY(c->h_nwin.resize(1));
    c->h_plan_status[0] = 0;
    CopySpans sp; /* one launch for all of them */
    auto d2h = [&](auto &vec, const void *src, size_t bytes) -> hipError_t {
        void *d = nullptr;
        const hipError_t e = vec.device_ptr(0, &d);
        if (e == hipSuccess)
            sp.add(d, src, bytes);
        return e;
    };
    if (c->plan_status.p)
        HIP_TRY(d2h(c->h_plan_status, c->plan_status.p, sizeof(uint32_t)));
    HIP_TRY(d2h(c->h_nwin, c->wbase.as<uint64_t>() + n_seq, sizeof(uint64_t)));
    if (n_seq) {
        HIP_TRY(d2h(c->h_hcount, c->hit_count.p, n_seq * sizeof(uint32_t)));
        HIP_TRY(d2h(c->h_ccount, c->call_count.p, n_seq * sizeof(uint32_t)));
        if (want_otu)
            HIP_TRY(d2h(c->h_ocount, c->otu_count.p, n_seq * sizeof(uint32_t)));
    }
    if (want_best && n_seq && !need_hits && !want_calls && !want_otu) {
        HIP_TRY(c->h_best.resize(n_seq));
        HIP_TRY(d2h(c->h_best, c->best.p, n_seq * sizeof(kgx_best_call)));
    }
    HIP_TRY(launch_copy_spans(sp, 64, c->stream));
    c->counts_enqueued = want + 1;
    return KGX_OK;
}

/* One pass over a whole host batch, split so that a pool can enqueue its
 * shards in order from one thread and collect them on several: the staging
 * (or, for residues in the caller's pinned memory, nothing) and the upload by
 * pull kernels -- on `up` with `up_done` recorded, which the context's stream
 * waits for, when given, else on the context's stream -- then the device pass
 * (plan, probe, score).  A caller-pinned batch is NUL-scanned on the device. */
int one_pass_enqueue(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                     uint32_t n_seq, uint32_t want, hipStream_t up, hipEvent_t up_done, HostPool *stage)
{
    const uint64_t r0 = n_seq ? seq_offsets[0] : 0, n_res = n_seq ? seq_offsets[n_seq] - r0 : 0;
    /* the residues to copy: the caller's pinned buffer, or our staging */
    const void *src = residues + r0;
    const bool pin = c->opt.pinned_input && host_pinned_range(residues + r0, n_res);
    c->one_pass_pinned = pin;
    if (pin) {
        HIP_TRY(c->h_off_stage.resize(n_seq + 1));
        stage_offsets_into(c->h_off_stage.data(), seq_offsets, 0, n_seq);
        c->pinned_batches++;
    } else {
        HostPool *sp = stage;
        if (!sp && n_res >= (1u << 20))
            sp = ensure_stage_pool(c);
        if (int rc = stage_host_copy(c, residues, seq_offsets, 0, n_seq, sp))
            return rc;
        src = c->h_res.data();
    }
    /* up by DMA, the small copy first (the DMA engine serves every stream in
     * order).  With `up` the copies go on that stream and the context's
     * stream waits for an event: a pool enqueues its shards' uploads on one
     * such stream and their passes in shard order, so a hardware queue shared
     * by two shards' streams never holds a shard's kernels behind a later
     * shard's upload (r5o: per-shard threads uploading on their own streams
     * at once did).  Uploads by kernels reading the mapped memory instead
     * measured worse: the device's PCIe reads held up the other shards'
     * kernels (r5q/r5r: a 10-us plan kernel took 140 us beside them). */
    HIP_TRY(c->residues.reserve(n_res + 16));
    HIP_TRY(c->offsets.reserve((n_seq + 1) * sizeof(uint64_t)));
    hipStream_t us = up ? up : c->stream;
    HIP_TRY(hipMemcpyAsync(c->offsets.p, c->h_off_stage.data(), (n_seq + 1) * sizeof(uint64_t),
                           hipMemcpyHostToDevice, us));
    if (n_res)
        HIP_TRY(hipMemcpyAsync(c->residues.p, src, n_res, hipMemcpyHostToDevice, us));
    if (up) {
        HIP_TRY(hipEventRecord(up_done, up));
        HIP_TRY(hipStreamWaitEvent(c->stream, up_done, 0));
    }
    if (pin) {
        HIP_TRY(c->h_nul.resize(1));
        c->h_nul[0] = 0;
        void *dn = nullptr;
        HIP_TRY(c->h_nul.device_ptr(0, &dn));
        HIP_TRY(launch_nul_scan(c->residues.as<uint8_t>(), 0, n_res, static_cast<uint32_t *>(dn), c->stream));
    }
    /* on the wave scorer, the host knows whether any sequence needs the lane
     * machine's long-sequence pass (score_long): usually none does */
    const int variant = c->opt.score_variant;
    if (c->opt.score_variant == SCORE_WAVE) {
        uint64_t longest = 0;
        for (uint32_t s = 0; s < n_seq; s++)
            longest = std::max(longest, seq_offsets[s + 1] - seq_offsets[s]);
        if (windows_of(longest) <= (uint64_t)RUN_CAP)
            c->opt.score_variant = SCORE_WAVE_ONLY;
    }
    const int rc = kgx_run_device(c, params, c->residues.as<uint8_t>(), c->offsets.as<uint64_t>(), n_seq, n_res,
                                  want, nullptr);
    c->opt.score_variant = variant;
    return rc;
}

/* the enqueued pass's results (kgx_device_batch_collect); a caller-pinned
 * batch whose scan found a NUL runs again, staged and cut at the NUL */
int one_pass_collect(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                     uint32_t n_seq, uint32_t want, kgx_result *out)
{
    int rc = kgx_device_batch_collect(c, want, out);
    if (!rc && c->one_pass_pinned && __atomic_load_n(&c->h_nul[0], __ATOMIC_ACQUIRE)) {
        c->nul_reruns++;
        c->opt.pinned_input = 0;
        rc = one_pass_enqueue(c, params, residues, seq_offsets, n_seq, want, nullptr, nullptr);
        if (!rc)
            rc = kgx_device_batch_collect(c, want, out);
        c->opt.pinned_input = 1;
    }
    return rc;
}

}  // namespace kgx
}  // extern "C++"

namespace {

/* the context's own expansion (into h_hits, CSR numbering): R12 records of
 * hit j at h_hits12 + 3 (j + rec_delta), else h_hits16[j + rec_delta]; the
 * chunk's mask from h_mask + mbase */
int expand_hits(bool R12, kgx_ctx *c, const char *residues, const uint64_t *seq_offsets, uint32_t a, uint32_t b,
                uint64_t mbase, int64_t rec_delta)
{
    kgx_hit_chunk ch{};
    ch.seq_begin = 0;
    ch.record_words = R12 ? 3 : 4;
    ch.hit_begin = 0;
    ch.records = R12 ? c->h_hits12.data() + 3 * rec_delta
                     : reinterpret_cast<const uint32_t *>(c->h_hits16.data() + rec_delta);
    ch.mask = c->h_mask.data() + mbase;
    ch.window_start = c->h_wstart.data();
    return expand_chunk(ch, c->h_hoff.data(), residues, seq_offsets, a, b, c->h_hits.data(), 0, 0, c->opt.host_nt != 0);
}

}  // namespace
}  // extern "C"

/* ---- what the streamed and the exact chunk schedule share ---- */

namespace {

using Clock = std::chrono::steady_clock;
inline Clock::time_point now() { return Clock::now(); }
inline double ms(Clock::time_point a, Clock::time_point b)
{
    return std::chrono::duration<double, std::milli>(b - a).count();
}

/* h_wstart: each sequence's first window relative to its chunk (chunk k =
 * sequences [cut[k], cut[k + 1])); returns the chunks' window totals */
std::vector<uint64_t> chunk_window_starts(kgx_ctx *c, const uint64_t *seq_offsets, uint32_t n_seq,
                                          const std::vector<uint32_t> &cut, uint32_t K)
{
    std::vector<uint64_t> win(K, 0);
    c->h_wstart.resize(n_seq);
    for (uint32_t k = 0; k < K; k++) {
        uint64_t w = 0;
        for (uint32_t s = cut[k]; s < cut[k + 1]; s++) {
            c->h_wstart[s] = w;
            w += windows_of(seq_offsets[s + 1] - seq_offsets[s]);
        }
        win[k] = w;
    }
    return win;
}

/* the host arrays of a chunked batch's results, empty */
int reset_chunked_results(kgx_ctx *c, uint32_t n_seq, bool want_best, bool compact)
{
    c->h_hoff.assign(n_seq + 1, 0);
    c->h_coff.assign(n_seq + 1, 0);
    c->h_ooff.assign(n_seq + 1, 0);
    HIP_TRY(c->h_hits.resize(0));
    HIP_TRY(c->h_calls.resize(0));
    HIP_TRY(c->h_otus.resize(0));
    HIP_TRY(c->h_best.resize(want_best ? n_seq : 0));
    if (compact) {
        HIP_TRY(c->h_hits16.resize(0));
        HIP_TRY(c->h_mask.resize(0));
    }
    return KGX_OK;
}

/* a chunk's hit mask (nwords) / best calls (n sequences) into x's dense
 * buffers, on x's stream: chunk k+2's kernels overwrite the originals before
 * chunk k's bulk copy has read them */
int keep_mask(kgx_ctx *x, uint64_t nwords)
{
    if (nwords) {
        HIP_TRY(x->dense_mask.reserve(nwords * sizeof(uint64_t)));
        HIP_TRY(launch_copy_to_host(x->dense_mask.p, x->hit_mask.p, nwords * sizeof(uint64_t), 256, x->stream));
    }
    return KGX_OK;
}
int keep_best(kgx_ctx *x, uint32_t n)
{
    if (n) {
        HIP_TRY(x->dense_best.reserve(n * sizeof(kgx_best_call)));
        HIP_TRY(hipMemcpyAsync(x->dense_best.p, x->best.p, n * sizeof(kgx_best_call), hipMemcpyDeviceToDevice,
                               x->stream));
    }
    return KGX_OK;
}

/* Host threads expand the compact records of chunk k (sequences [s0, s0 + n),
 * h_hoff final for them) in up to pool-size hit-balanced sequence ranges,
 * while the next chunks stream.  The streamed schedule submits a chunk whose
 * records have landed, record j at j + rec_delta (landed null); the exact one
 * submits at once and each task waits for the chunk's bulk copy (landed). */
void submit_expansion(kgx_ctx *c, bool r12, const char *residues, const uint64_t *seq_offsets, uint32_t k,
                      uint32_t s0, uint32_t n, uint64_t mbase, int64_t rec_delta, hipEvent_t landed,
                      std::atomic<uint64_t> *expand_ns)
{
    const bool timing = std::getenv("KGX_TIMING") != nullptr;
    const uint64_t h0 = c->h_hoff[s0], nh = c->h_hoff[s0 + n] - h0;
    const uint32_t P = c->pool->size();
    uint32_t a = s0;
    for (uint32_t p = 1; p <= P && a < s0 + n; p++) {
        uint32_t b = s0 + n;
        if (p < P) {
            const uint64_t target = h0 + nh * p / P;
            b = (uint32_t)(std::lower_bound(c->h_hoff.begin() + a, c->h_hoff.begin() + s0 + n, target) -
                           c->h_hoff.begin());
            b = std::max(b, a + 1);
        }
        c->pool->submit([=]() -> int {
            const auto q0 = now();
            if (landed) {
                const hipError_t e = hipEventSynchronize(landed);
                if (e != hipSuccess)
                    return fail(KGX_EDEVICE, std::string("chunk event: ") + hipGetErrorString(e));
            }
            const auto q1 = now();
            const int erc = expand_hits(r12, c, residues, seq_offsets, a, b, mbase, rec_delta);
            if (expand_ns)
                *expand_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(now() - q0).count();
            if (timing && landed)
                std::fprintf(stderr, "[kgx] chunk %u expand [%u,%u): wait %.3f ms, expand %.3f ms\n", k, a, b,
                             ms(q0, q1), ms(q1, now()));
            else if (timing)
                std::fprintf(stderr, "[kgx] streamed chunk %u expand [%u,%u): %.3f ms\n", k, a, b, ms(q0, now()));
            return erc;
        });
        a = b;
    }
}

}  // namespace

extern "C" {
namespace {

/* Streamed host batch (compact records, PACKED16 images): no host round
 * trip inside a chunk.  Each chunk runs on its context's stream as
 *   H2D -> plan/probe/score -> count scan (device CSR offsets) -> gather
 *   into dense buffers (+ mask, counts, best calls)
 * and its bulk device-to-host copy runs on the copy stream, sized on the
 * device (the scanned totals) into host regions whose room the host set from
 * the chunk's window count and the hit / call / OTU rates seen so far.  The
 * host enqueues every chunk up front (each context's staging buffer is
 * reused once its H2D is done), then, chunk by chunk as the copies land,
 * builds the CSR offsets from the counts, moves calls / OTUs into place and
 * hands the records to the expansion threads.  A chunk whose results did not
 * fit its region makes the call return STREAM_OVERFLOW after raising the rates;
 * the caller reruns the batch on the exact (host round trip) path. */
constexpr int STREAM_OVERFLOW = 1; /* internal: a region overflowed, rerun exact */
constexpr int STREAM_NUL = 2;      /* internal: the caller's pinned residues hold a NUL, rerun staged */

int process_batch_streamed(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                           uint32_t n_seq, uint32_t want, uint32_t K, const std::vector<uint32_t> &cut,
                           kgx_result *out)
{
    kgx_ctx *t = c->twin;
    kgx_ctx *xs[2] = {c, t};
    const bool want_calls = (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = (want & KGX_WANT_OTU) != 0;
    const bool want_best = (want & KGX_WANT_BEST) != 0;
    const bool timing = std::getenv("KGX_TIMING") != nullptr;
    const auto T0 = now();
    int rc = KGX_OK;

    /* per-chunk windows, regions and offsets */
    std::vector<uint64_t> cap_h(K), cap_c(K), cap_o(K), rb_h(K + 1, 0), rb_c(K + 1, 0), rb_o(K + 1, 0), mb(K + 1, 0);
    const std::vector<uint64_t> win = chunk_window_starts(c, seq_offsets, n_seq, cut, K);
    for (uint32_t k = 0; k < K; k++) {
        const uint64_t w = win[k];
        /* region starts stay 16-B aligned: multiples of 4 records */
        auto room = [w](double rate, uint64_t extra) {
            return (std::min<uint64_t>(w, (uint64_t)(rate * (double)w) + extra) + 3) & ~3ull;
        };
        cap_h[k] = room(c->rate_hits, 256);
        cap_c[k] = want_calls ? room(c->rate_calls, 64) : 0;
        cap_o[k] = want_otu ? room(c->rate_otus, 64) : 0;
        rb_h[k + 1] = rb_h[k] + cap_h[k];
        rb_c[k + 1] = rb_c[k] + cap_c[k];
        rb_o[k + 1] = rb_o[k] + cap_o[k];
        mb[k + 1] = mb[k] + (((w + 63) / 64 + 1) & ~1ull); /* 16-B aligned mask regions */
    }
    /* pinned host regions: resized before any copy or expansion is in flight */
    const bool r12 = c->opt.host_rec12 != 0;
    if (r12)
        HIP_TRY(c->h_hits12.resize(3 * rb_h[K]));
    else
        HIP_TRY(c->h_hits16.resize(rb_h[K]));
    HIP_TRY(c->h_mask.resize(mb[K]));
    HIP_TRY(c->h_calls_region.resize(rb_c[K]));
    HIP_TRY(c->h_otus_region.resize(rb_o[K]));
    HIP_TRY(c->h_counts.resize(3 * (uint64_t)n_seq));
    const bool expand = !c->compact_out;
    if (expand)
        HIP_TRY(c->h_hits.resize(rb_h[K])); /* room for every region's records; trimmed below */
    /* host_profile: timing events per chunk (4 on the contexts' streams, 1 on the copy stream) */
    const bool prof = c->opt.host_profile != 0;
    if (prof && ((rc = ensure_events(c->prof_ev, 4 * (size_t)K, hipEventDefault)) ||
                 (rc = ensure_events(c->prof_done, K, hipEventDefault))))
        return rc;
    double stage_ms = 0;
    std::atomic<uint64_t> expand_ns{0};
    c->compact_segs.clear();
    HIP_TRY(c->h_best.resize(want_best ? n_seq : 0));
    c->h_hoff.assign(n_seq + 1, 0);
    c->h_coff.assign(n_seq + 1, 0);
    c->h_ooff.assign(n_seq + 1, 0);

    /* device buffers of both contexts at the largest chunk's size up front:
     * no reallocation while earlier chunks still read them */
    uint64_t max_res = 1, max_n = 1;
    for (uint32_t k = 0; k < K; k++) {
        max_res = std::max(max_res, seq_offsets[cut[k + 1]] - seq_offsets[cut[k]]);
        max_n = std::max<uint64_t>(max_n, cut[k + 1] - cut[k]);
    }
    for (kgx_ctx *x : xs) {
        HIP_TRY(x->residues.reserve(max_res + 16));
        HIP_TRY(x->offsets.reserve((max_n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->dense_hoff.reserve((max_n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->dense_coff.reserve((max_n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->dense_ooff.reserve((max_n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->cscan_ws.reserve(count_scan_workspace_bytes((uint32_t)max_n)));
        HIP_TRY(x->dense_hits.reserve(max_res * 16));
        if (want_calls)
            HIP_TRY(x->dense_calls.reserve(max_res * sizeof(kgx_call)));
        if (want_otu)
            HIP_TRY(x->dense_otus.reserve(max_res * sizeof(kgx_otu)));
        HIP_TRY(x->dense_mask.reserve((max_res / 64 + 2) * sizeof(uint64_t)));
        HIP_TRY(x->dense_counts.reserve(3 * max_n * sizeof(uint32_t)));
        if (want_best)
            HIP_TRY(x->dense_best.reserve(max_n * sizeof(kgx_best_call)));
    }

    hipStream_t cs = c->copy_stream;
    const int cb = c->opt.host_copy_blocks;
    auto mapped = [](auto &v, uint64_t at, void **d) -> hipError_t { return v.device_ptr(at, d); };
    /* host_upload_stream: each chunk's regions of up_res (256-B aligned, 16
     * bytes of slack for the probe's 16-B residue loads) and up_off */
    const bool up = c->opt.host_upload_stream != 0;
    std::vector<uint64_t> res_at(K + 1, 0), off_at(K + 1, 0);
    for (uint32_t k = 0; k < K; k++) {
        res_at[k + 1] = res_at[k] + ((seq_offsets[cut[k + 1]] - seq_offsets[cut[k]] + 16 + 255) & ~255ull);
        off_at[k + 1] = off_at[k] + ((cut[k + 1] - cut[k] + 1 + 1) & ~1ull);
    }
    if (up) {
        HIP_TRY(c->up_res.reserve(std::max<uint64_t>(res_at[K], 256)));
        HIP_TRY(c->up_off.reserve(std::max<uint64_t>(off_at[K], 2) * sizeof(uint64_t)));
    }
    /* host_stage_all: every chunk staged into a pinned region of its own (the
     * same res_at / off_at layout), so no staging waits for the H2D of the
     * chunk two before to free its context's staging buffer */
    const bool sall = c->opt.host_stage_all != 0;
    if (sall) {
        HIP_TRY(c->h_res_all.resize(std::max<uint64_t>(res_at[K], 256)));
        HIP_TRY(c->h_off_all.resize(std::max<uint64_t>(off_at[K], 2)));
    }
    /* caller-pinned residues: no staging copy, a device NUL scan instead */
    const uint64_t all_res = n_seq ? seq_offsets[n_seq] - seq_offsets[0] : 0;
    const bool pin = c->opt.pinned_input && host_pinned_range(residues + (n_seq ? seq_offsets[0] : 0), all_res);
    uint32_t *d_nul = nullptr;
    if (pin) {
        HIP_TRY(c->h_nul.resize(1));
        c->h_nul[0] = 0;
        void *dn = nullptr;
        HIP_TRY(c->h_nul.device_ptr(0, &dn));
        d_nul = static_cast<uint32_t *>(dn);
        c->pinned_batches++;
    }
    auto staged_res = [&](kgx_ctx *x, uint32_t k) -> const char * {
        if (pin)
            return residues + seq_offsets[cut[k]];
        return sall ? c->h_res_all.data() + res_at[k] : x->h_res.data();
    };
    auto staged_off = [&](kgx_ctx *x, uint32_t k) -> const uint64_t * {
        return sall ? c->h_off_all.data() + off_at[k] : x->h_off_stage.data();
    };

    /* enqueue chunk k on x: everything up to its bulk copy */
    auto enqueue = [&](kgx_ctx *x, uint32_t k) -> int {
        const uint32_t s0 = cut[k], n = cut[k + 1] - cut[k];
        const uint64_t n_res = n ? seq_offsets[cut[k + 1]] - seq_offsets[s0] : 0;
        const char *hres = staged_res(x, k);
        const uint64_t *hoff = staged_off(x, k);
        hipStream_t us = up ? c->up_stream : x->stream;
        if (prof)
            HIP_TRY(hipEventRecord(c->prof_ev[4 * k], us));
        const uint8_t *d_res = x->residues.as<uint8_t>();
        const uint64_t *d_off = x->offsets.as<uint64_t>();
        int rc = KGX_OK;
        if (up) {
            uint8_t *rd = c->up_res.as<uint8_t>() + res_at[k];
            uint64_t *od = c->up_off.as<uint64_t>() + off_at[k];
            HIP_TRY(hipMemcpyAsync(od, hoff, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, us));
            if (n_res)
                HIP_TRY(hipMemcpyAsync(rd, hres, n_res, hipMemcpyHostToDevice, us));
            d_res = rd;
            d_off = od;
        } else {
            /* reserved for the largest chunk above: no reallocation here */
            HIP_TRY(x->residues.reserve(n_res + 16));
            HIP_TRY(x->offsets.reserve((n + 1) * sizeof(uint64_t)));
            HIP_TRY(hipMemcpyAsync(x->offsets.p, hoff, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, us));
            if (n_res)
                HIP_TRY(hipMemcpyAsync(x->residues.p, hres, n_res, hipMemcpyHostToDevice, us));
        }
        HIP_TRY(hipEventRecord(c->chunk_h2d[k], us));
        if (pin)
            HIP_TRY(launch_nul_scan(d_res, 0, n_res, d_nul, us));
        if (prof)
            HIP_TRY(hipEventRecord(c->prof_ev[4 * k + 1], us));
        if (up)
            HIP_TRY(hipStreamWaitEvent(x->stream, c->chunk_h2d[k], 0));
        if ((rc = kgx_run_device(x, params, d_res, d_off, n, n_res, want, nullptr)))
            return rc;
        if (prof)
            HIP_TRY(hipEventRecord(c->prof_ev[4 * k + 2], x->stream));
        const uint64_t rn = std::max<uint64_t>(n_res, 1); /* dense buffers: at most one record per residue */
        HIP_TRY(x->dense_hoff.reserve((n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->dense_coff.reserve((n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->dense_ooff.reserve((n + 1) * sizeof(uint64_t)));
        HIP_TRY(x->cscan_ws.reserve(count_scan_workspace_bytes(n)));
        /* x's dense buffers still feed chunk k-2's bulk copy, and so do its
         * scanned totals (dense_hoff/coff/ooff + n, read by the counted copies
         * when they run): nothing of chunk k touches them before that is done */
        if (k >= 2)
            HIP_TRY(hipStreamWaitEvent(x->stream, c->chunk_done[k - 2], 0));
        HIP_TRY(launch_count_scan(n, x->hit_count.as<uint32_t>(), want_calls ? x->call_count.as<uint32_t>() : nullptr,
                                  want_otu ? x->otu_count.as<uint32_t>() : nullptr, x->dense_hoff.as<uint64_t>(),
                                  x->dense_coff.as<uint64_t>(), x->dense_ooff.as<uint64_t>(), x->cscan_ws.p,
                                  x->stream));
        HIP_TRY(x->dense_hits.reserve(rn * 16));
        if (want_calls)
            HIP_TRY(x->dense_calls.reserve(rn * sizeof(kgx_call)));
        if (want_otu)
            HIP_TRY(x->dense_otus.reserve(rn * sizeof(kgx_otu)));
        HIP_TRY(launch_gather(n, x->wbase.as<uint64_t>(), x->hit_mask.as<uint64_t>(), x->tile_windows,
                              x->call_count.as<uint32_t>(), x->hits.as<uint4>(), x->hits.as<uint4>() + x->hit_slots,
                              x->calls.as<kgx_call>(), x->dense_hoff.as<uint64_t>(), x->dense_coff.as<uint64_t>(),
                              nullptr, want_calls ? x->dense_calls.as<kgx_call>() : nullptr, s0, x->hit_format,
                              x->otu_count.as<uint32_t>(), x->otus.as<kgx_otu>(), x->dense_ooff.as<uint64_t>(),
                              want_otu ? x->dense_otus.as<kgx_otu>() : nullptr, x->stream,
                              r12 ? nullptr : x->dense_hits.as<uint4>(), r12 ? x->dense_hits.as<uint32_t>() : nullptr));
        /* what chunk k+2's kernels overwrite: mask, counts, best calls */
        if ((rc = keep_mask(x, (win[k] + 63) / 64)))
            return rc;
        if (n) {
            HIP_TRY(x->dense_counts.reserve(3 * (uint64_t)n * sizeof(uint32_t)));
            uint32_t *dc = x->dense_counts.as<uint32_t>();
            HIP_TRY(launch_copy_to_host(dc, x->hit_count.p, n * sizeof(uint32_t), 64, x->stream));
            if (want_calls)
                HIP_TRY(launch_copy_to_host(dc + n, x->call_count.p, n * sizeof(uint32_t), 64, x->stream));
            if (want_otu)
                HIP_TRY(launch_copy_to_host(dc + 2 * (uint64_t)n, x->otu_count.p, n * sizeof(uint32_t), 64, x->stream));
        }
        if (want_best && (rc = keep_best(x, n)))
            return rc;
        HIP_TRY(hipEventRecord(c->chunk_gathered[k], x->stream));
        if (prof)
            HIP_TRY(hipEventRecord(c->prof_ev[4 * k + 3], x->stream));
        return KGX_OK;
    };

    /* chunk k's bulk copy, on the copy stream, issued once chunk k+1 is
     * enqueued: with option host_h2d_first it also waits for chunk k+1's
     * residues to be on the device.  A chunk's H2D beside a running D2H of
     * device stores crawled (r4c: 5 MB in 0.36 ms against 0.10 alone -- its
     * read requests queue behind the posted writes upstream), and the next
     * chunk's kernels waited for it; the D2H loses nothing by starting the
     * H2D's ~0.1 ms later. */
    auto copy_out = [&](kgx_ctx *x, uint32_t k) -> int {
        const uint32_t s0 = cut[k], n = cut[k + 1] - cut[k];
        const uint64_t nwords = (win[k] + 63) / 64;
        HIP_TRY(hipStreamWaitEvent(cs, c->chunk_gathered[k], 0));
        if (c->opt.host_h2d_first && k + 1 < K)
            HIP_TRY(hipStreamWaitEvent(cs, c->chunk_h2d[k + 1], 0));
        void *d = nullptr;
        if (c->opt.host_stream_dma) {
            /* DMA engines, sized on the host: every region copied whole */
            auto dma = [&](void *dst, const void *src, uint64_t bytes) -> hipError_t {
                return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, cs) : hipSuccess;
            };
            const uint32_t planes = want_otu ? 3 : want_calls ? 2 : 1;
            HIP_TRY(dma(c->h_counts.data() + 3 * (uint64_t)s0, x->dense_counts.p, planes * (uint64_t)n * sizeof(uint32_t)));
            if (r12)
                HIP_TRY(dma(c->h_hits12.data() + 3 * rb_h[k], x->dense_hits.p, cap_h[k] * 12));
            else
                HIP_TRY(dma(c->h_hits16.data() + rb_h[k], x->dense_hits.p, cap_h[k] * 16));
            HIP_TRY(dma(c->h_mask.data() + mb[k], x->dense_mask.p, nwords * sizeof(uint64_t)));
            if (want_calls)
                HIP_TRY(dma(c->h_calls_region.data() + rb_c[k], x->dense_calls.p, cap_c[k] * sizeof(kgx_call)));
            if (want_otu)
                HIP_TRY(dma(c->h_otus_region.data() + rb_o[k], x->dense_otus.p, cap_o[k] * sizeof(kgx_otu)));
            if (want_best)
                HIP_TRY(dma(c->h_best.data() + s0, x->dense_best.p, n * sizeof(kgx_best_call)));
            HIP_TRY(hipEventRecord(c->chunk_done[k], cs));
            if (prof)
                HIP_TRY(hipEventRecord(c->prof_done[k], cs));
            return KGX_OK;
        }
        if (n) {
            const uint32_t planes = want_otu ? 3 : want_calls ? 2 : 1;
            HIP_TRY(mapped(c->h_counts, 3 * (uint64_t)s0, &d));
            HIP_TRY(launch_copy_to_host(d, x->dense_counts.p, planes * (uint64_t)n * sizeof(uint32_t), cb, cs));
        }
        if (r12)
            HIP_TRY(mapped(c->h_hits12, 3 * rb_h[k], &d));
        else
            HIP_TRY(mapped(c->h_hits16, rb_h[k], &d));
        HIP_TRY(launch_copy_counted(d, x->dense_hits.p, x->dense_hoff.as<uint64_t>() + n, cap_h[k], r12 ? 12 : 16,
                                    cb, cs));
        if (nwords) {
            HIP_TRY(mapped(c->h_mask, mb[k], &d));
            HIP_TRY(launch_copy_to_host(d, x->dense_mask.p, nwords * sizeof(uint64_t), cb, cs));
        }
        if (want_calls && cap_c[k]) {
            HIP_TRY(mapped(c->h_calls_region, rb_c[k], &d));
            HIP_TRY(launch_copy_counted(d, x->dense_calls.p, x->dense_coff.as<uint64_t>() + n, cap_c[k],
                                        sizeof(kgx_call), cb, cs));
        }
        if (want_otu && cap_o[k]) {
            HIP_TRY(mapped(c->h_otus_region, rb_o[k], &d));
            HIP_TRY(launch_copy_counted(d, x->dense_otus.p, x->dense_ooff.as<uint64_t>() + n, cap_o[k],
                                        sizeof(kgx_otu), cb, cs));
        }
        if (want_best && n) {
            HIP_TRY(mapped(c->h_best, s0, &d));
            HIP_TRY(launch_copy_to_host(d, x->dense_best.p, n * sizeof(kgx_best_call), cb, cs));
        }
        HIP_TRY(hipEventRecord(c->chunk_done[k], cs));
        if (prof)
            HIP_TRY(hipEventRecord(c->prof_done[k], cs));
        return KGX_OK;
    };

    /* chunk k's results on the host -> CSR offsets, calls / OTUs in place,
     * expansion tasks; false in *fits when a region overflowed */
    uint64_t hbase = 0, cbase = 0, obase = 0, nwin = 0;
    double max_rh = 0, max_rc = 0, max_ro = 0;
    bool fits = true;
    auto collect = [&](uint32_t k) -> int {
        HIP_TRY(hipEventSynchronize(c->chunk_done[k]));
        const uint32_t s0 = cut[k], n = cut[k + 1] - cut[k];
        const uint32_t *hc = c->h_counts.data() + 3 * (uint64_t)s0, *cc = hc + n, *oc = hc + 2 * (uint64_t)n;
        uint64_t nh = 0, nc = 0, no = 0;
        for (uint32_t i = 0; i < n; i++) {
            nh += hc[i];
            nc += want_calls ? cc[i] : 0;
            no += want_otu ? oc[i] : 0;
            c->h_hoff[s0 + i + 1] = hbase + nh;
            c->h_coff[s0 + i + 1] = cbase + nc;
            c->h_ooff[s0 + i + 1] = obase + no;
        }
        nwin += win[k];
        if (win[k]) {
            max_rh = std::max(max_rh, (double)nh / (double)win[k]);
            max_rc = std::max(max_rc, (double)nc / (double)win[k]);
            max_ro = std::max(max_ro, (double)no / (double)win[k]);
        }
        if (nh > cap_h[k] || nc > cap_c[k] || no > cap_o[k])
            fits = false;
        if (fits) {
            if (nc)
                std::memmove(c->h_calls_region.data() + cbase, c->h_calls_region.data() + rb_c[k],
                             nc * sizeof(kgx_call));
            if (no)
                std::memmove(c->h_otus_region.data() + obase, c->h_otus_region.data() + rb_o[k],
                             no * sizeof(kgx_otu));
            if (nh && !expand) {
                /* compact results: the records stay where they landed */
                c->compact_segs.push_back({s0, s0 + n, r12 ? 3u : 4u, hbase, rb_h[k], mb[k]});
            } else if (nh) {
                submit_expansion(c, r12, residues, seq_offsets, k, s0, n, mb[k], (int64_t)rb_h[k] - (int64_t)hbase,
                                 nullptr, &expand_ns);
            }
        }
        hbase += nh;
        cbase += nc;
        obase += no;
        return KGX_OK;
    };

    HostPool *sp = ensure_stage_pool(c);
    uint32_t next = 0; /* next chunk to collect */
    /* KGX_TIMING: the host's own clock per chunk (ms from T0): staging
     * entered / staged / enqueued, and each collect's end */
    std::vector<double> ht;
    for (uint32_t k = 0; k < K && !rc; k++) {
        kgx_ctx *x = xs[k & 1];
        if (k >= 2 && !sall)
            HIP_TRY(hipEventSynchronize(c->chunk_h2d[k - 2])); /* x's staging buffer is free */
        const auto ts = now();
        if (pin && sall)
            stage_offsets_into(c->h_off_all.data() + off_at[k], seq_offsets, cut[k], cut[k + 1]);
        else if (pin) {
            if (x->h_off_stage.resize(cut[k + 1] - cut[k] + 1) != hipSuccess)
                rc = fail(KGX_ENOMEM, "pinned staging");
            else
                stage_offsets_into(x->h_off_stage.data(), seq_offsets, cut[k], cut[k + 1]);
        } else if (sall)
            stage_copy_into(c->h_res_all.data() + res_at[k], c->h_off_all.data() + off_at[k], residues, seq_offsets,
                            cut[k], cut[k + 1], sp);
        else
            rc = stage_host_copy(x, residues, seq_offsets, cut[k], cut[k + 1], sp);
        const auto te = now();
        stage_ms += ms(ts, te);
        if (rc || (rc = enqueue(x, k)))
            break;
        if (k >= 1 && (rc = copy_out(xs[(k - 1) & 1], k - 1)))
            break;
        if (timing)
            ht.insert(ht.end(), {(double)k, ms(T0, ts), ms(T0, te), ms(T0, now())});
        /* collect what has landed meanwhile */
        while (!rc && next < k && hipEventQuery(c->chunk_done[next]) == hipSuccess) {
            rc = collect(next++);
            if (timing)
                ht.insert(ht.end(), {-1.0 - (double)(next - 1), ms(T0, now()), 0.0, 0.0});
        }
    }
    if (!rc && K)
        rc = copy_out(xs[(K - 1) & 1], K - 1);
    while (!rc && next < K) {
        rc = collect(next++);
        if (timing)
            ht.insert(ht.end(), {-1.0 - (double)(next - 1), ms(T0, now()), 0.0, 0.0});
    }
    for (size_t i = 0; timing && i + 3 < ht.size(); i += 4) {
        if (ht[i] >= 0)
            std::fprintf(stderr, "[kgx] host chunk %d: stage %.3f-%.3f, enqueued %.3f ms\n", (int)ht[i], ht[i + 1],
                         ht[i + 2], ht[i + 3]);
        else
            std::fprintf(stderr, "[kgx] host collect %d done %.3f ms\n", (int)(-ht[i] - 1), ht[i + 1]);
    }
    /* drain everything, whatever happened above */
    const hipError_t e0 = hipStreamSynchronize(xs[0]->stream), e1 = hipStreamSynchronize(xs[1]->stream);
    hipError_t e2 = hipStreamSynchronize(cs);
    if (c->up_stream) { /* an upload issued before a failed enqueue may still read the staging memory */
        const hipError_t e3 = hipStreamSynchronize(c->up_stream);
        if (e2 == hipSuccess)
            e2 = e3;
    }
    const int prc = c->pool->wait();
    if (rc)
        return rc;
    HIP_TRY(e0);
    HIP_TRY(e1);
    HIP_TRY(e2);
    if (prc)
        return prc;
    if (pin && __atomic_load_n(&c->h_nul[0], __ATOMIC_ACQUIRE))
        return STREAM_NUL;
    /* the rates the next batch's regions are sized by */
    c->rate_hits = std::max(0.02, max_rh * 1.25);
    c->rate_calls = std::max(0.01, max_rc * 1.25);
    c->rate_otus = std::max(0.01, max_ro * 1.25);
    if (!fits)
        return STREAM_OVERFLOW;
    if (expand)
        HIP_TRY(c->h_hits.resize(hbase));
    c->have_hits = false;
    t->have_hits = false;
    if (timing)
        std::fprintf(stderr, "[kgx] streamed batch: %u chunks, %.3f ms\n", K, ms(T0, now()));
    if (prof) {
        kgx_host_profile &P = c->last_profile;
        P = kgx_host_profile{};
        P.chunks = K;
        P.streamed = 1;
        P.wall_ms = ms(T0, now());
        P.stage_ms = stage_ms;
        P.expand_ms = (double)expand_ns.load() * 1e-6;
        P.h2d_bytes = seq_offsets[n_seq] - seq_offsets[0] + (uint64_t)(n_seq + K) * sizeof(uint64_t);
        for (uint32_t k = 0; k < K; k++) {
            float a = 0, b = 0, g = 0, d = 0;
            HIP_TRY(hipEventElapsedTime(&a, c->prof_ev[4 * k], c->prof_ev[4 * k + 1]));
            HIP_TRY(hipEventElapsedTime(&b, c->prof_ev[4 * k + 1], c->prof_ev[4 * k + 2]));
            HIP_TRY(hipEventElapsedTime(&g, c->prof_ev[4 * k + 2], c->prof_ev[4 * k + 3]));
            HIP_TRY(hipEventElapsedTime(&d, c->prof_ev[4 * k + 3], c->prof_done[k]));
            P.h2d_ms += a;
            P.device_ms += b;
            P.gather_ms += g;
            P.d2h_ms += d;
            if (timing) { /* the device's clock, from chunk 0's first event */
                float t0 = 0;
                HIP_TRY(hipEventElapsedTime(&t0, c->prof_ev[0], c->prof_ev[4 * k]));
                std::fprintf(stderr, "[kgx] device chunk %u: h2d %.3f, kernels %.3f, gather %.3f, d2h %.3f, done %.3f ms\n",
                             k, t0, t0 + a, t0 + a + b, t0 + a + b + g, t0 + a + b + g + d);
            }
        }
        const uint64_t recb = r12 ? 12 : 16;
        P.d2h_bytes = hbase * recb + cbase * sizeof(kgx_call) +
                      obase * sizeof(kgx_otu) + mb[K] * sizeof(uint64_t) + 3ull * n_seq * sizeof(uint32_t) +
                      (want_best ? (uint64_t)n_seq * sizeof(kgx_best_call) : 0);
    }
    out->best = want_best ? c->h_best.data() : nullptr;
    out->n_seq = n_seq;
    out->hit_offsets = c->h_hoff.data();
    out->hits = expand ? c->h_hits.data() : nullptr;
    out->call_offsets = c->h_coff.data();
    out->calls = c->h_calls_region.data();
    out->otu_offsets = c->h_ooff.data();
    out->otus = c->h_otus_region.data();
    out->n_windows = nwin;
    return KGX_OK;
}

/* A stream for the host path's bulk copies / uploads.  The runtime spreads a
 * process's streams over a few hardware queues (4 by default), each a FIFO
 * that blocks behind an event wait at its head, so the copy stream's waits
 * held up other streams' work queued behind them.  The copy stream is made at
 * the device's lowest priority: the runtime keeps a queue pool per priority,
 * so it shares a queue only with other copy streams.  (Round 4's full-CU-mask
 * stream got a queue of its own but faulted inside rocprofv3's finalisation
 * when a process exited with it alive, r5c; it is gone.)  KGX_OWN_QUEUES=0:
 * a plain stream. */
hipError_t own_queue_stream(int device, hipStream_t *s)
{
    (void)device;
    const char *e = std::getenv("KGX_OWN_QUEUES");
    if (!e || std::atoi(e) != 0) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest &&
            hipStreamCreateWithPriority(s, hipStreamNonBlocking, least) == hipSuccess)
            return hipSuccess;
        (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

/* The host batch in K residue-balanced chunks of whole sequences, alternating
 * between c and its twin context: while chunk k's hits are gathered and
 * copied to the host on one stream, chunk k+1 is staged, copied up, probed
 * and scored on the other.  The D2H of the hit records is the bulk of the
 * PCIe traffic, so the rest hides behind it.  Results are identical to the
 * one-pass path (per-sequence work never spans chunks). */
int process_batch_chunked(kgx_ctx *c, const kgx_params *params, const char *residues,
                          const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, uint32_t K,
                          kgx_result *out)
{
    if (!c->twin) {
        int rc = kgx_ctx_create(c->img, &c->twin);
        if (rc)
            return rc;
    }
    kgx_ctx *t = c->twin;
    t->opt.probe_variant = c->opt.probe_variant;
    t->opt.probe_j = c->opt.probe_j;
    t->opt.probe_filter = c->opt.probe_filter;
    t->opt.probe_serialize = c->opt.probe_serialize;
    t->opt.score_variant = c->opt.score_variant;
    t->opt.score_wave_tiles = c->opt.score_wave_tiles;
    t->opt.score_lean = c->opt.score_lean;
    kgx_ctx *xs[2] = {c, t};
    if (!c->copy_stream)
        HIP_TRY(own_queue_stream(c->img->device, &c->copy_stream));
    /* the upload stream only when asked for: each own-queue stream holds a
     * hardware queue of the process's few */
    if (c->opt.host_upload_stream && !c->up_stream)
        HIP_TRY(own_queue_stream(c->img->device, &c->up_stream));
    for (auto *ev : {&c->chunk_counts, &c->chunk_gathered, &c->chunk_done, &c->chunk_h2d})
        if (int erc = ensure_events(*ev, K))
            return erc;

    const uint64_t r0 = seq_offsets[0], n_res = seq_offsets[n_seq] - r0;
    std::vector<uint32_t> cut(K + 1, 0);
    cut[K] = n_seq;
    /* chunk weights: with host_taper the first and last chunks are half the
     * others (the first one's kernels and the last one's copy + expansion
     * are the parts of the batch nothing overlaps) */
    const bool taper = c->opt.host_taper && K >= 3;
    const double wsum = taper ? (double)K - 1.0 : (double)K;
    for (uint32_t k = 1; k < K; k++) {
        const double before = taper ? 0.5 + (double)(k - 1) : (double)k; /* weight of chunks < k */
        const uint64_t target = r0 + (uint64_t)((double)n_res * before / wsum);
        uint32_t s = (uint32_t)(std::lower_bound(seq_offsets, seq_offsets + n_seq + 1, target) - seq_offsets);
        cut[k] = std::min(std::max(s, cut[k - 1]), n_seq);
    }
    cut.erase(std::unique(cut.begin(), cut.end()), cut.end()); /* no empty chunks */
    K = (uint32_t)cut.size() - 1;
    const bool want_calls = (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = (want & KGX_WANT_OTU) != 0;
    const bool need_hits = (want & KGX_WANT_HITS) != 0;
    const bool want_best = (want & KGX_WANT_BEST) != 0;
    uint64_t hbase = 0, cbase = 0, obase = 0, nwin = 0;
    /* compact D2H: records + mask, expanded on the host pool */
    const bool compact = c->opt.host_hits16 && need_hits && c->img->layout == KGX_LAYOUT_PACKED16;
    uint64_t mbase = 0;
    int rc = reset_chunked_results(c, n_seq, want_best, compact);
    if (rc)
        return rc;
    struct PoolDrain { /* no expansion outlives this call, whatever path returns */
        HostPool *p = nullptr;
        ~PoolDrain()
        {
            if (p)
                (void)p->wait();
        }
    } drain;
    if (compact) {
        if (!c->pool || c->pool->size() != (unsigned)c->opt.host_threads)
            c->pool.reset(new HostPool((unsigned)c->opt.host_threads));
        drain.p = c->pool.get();
        if (c->opt.host_stream) {
            /* option host_score_variant: the scorer for the chunks (a chunk's
             * 17k sequences keep the lane scorer's long chains latency-bound;
             * the wave scorer is 1-3% faster per batch here, r4b) */
            const int sv_c = c->opt.score_variant, sv_t = t->opt.score_variant;
            if (c->opt.host_score_variant >= 0)
                c->opt.score_variant = t->opt.score_variant = c->opt.host_score_variant;
            const int src = process_batch_streamed(c, params, residues, seq_offsets, n_seq, want, K, cut, out);
            c->opt.score_variant = sv_c;
            t->opt.score_variant = sv_t;
            if (src != STREAM_OVERFLOW && src != STREAM_NUL)
                return src;
            /* a region overflowed (the rates are raised), or the caller's
             * pinned residues hold a NUL: this batch runs exact, staged */
            if (src == STREAM_NUL)
                c->nul_reruns++;
            if ((rc = reset_chunked_results(c, n_seq, want_best, compact)))
                return rc;
            c->compact_segs.clear();
            c->stream_fallbacks++;
        }
        chunk_window_starts(c, seq_offsets, n_seq, cut, K);
    }

    hipStream_t cs = c->copy_stream;

    /* device bytes -> the pinned result array at element `at`, on the copy
     * stream: device stores into the mapped memory (host_copy 1) or a DMA
     * copy */
    auto copy_out = [&](auto &dst, uint64_t at, const void *src, uint64_t n) -> int {
        if (!n)
            return KGX_OK;
        const uint64_t bytes = n * sizeof(dst[0]);
        if (c->opt.host_copy) {
            void *d = nullptr;
            HIP_TRY(dst.device_ptr(at, &d));
            HIP_TRY(launch_copy_to_host(d, src, bytes, c->opt.host_copy_blocks, cs));
        } else {
            HIP_TRY(hipMemcpyAsync(dst.data() + at, src, bytes, hipMemcpyDeviceToHost, cs));
        }
        return KGX_OK;
    };

    /* Schedule.  Each chunk runs H2D -> plan/probe/score -> counts D2H on its
     * context's stream (contexts alternate), then, once the host has turned
     * the counts into offsets, a gather into that context's dense buffers;
     * the bulk device-to-host copy of those buffers runs on a separate copy
     * stream, so chunk k+2's kernels on the same context are not held behind
     * chunk k's bulk copy (only chunk k+2's gather waits for it).
     * Device-to-host bytes cross PCIe in order, so chunk k+1's counts must
     * leave before chunk k's bulk (option counts_first): otherwise they queue
     * behind it and the host learns chunk k+1's sizes only once the link has
     * gone idle.  Chunks are staged and enqueued as soon as their context's
     * staging buffer is free, and host threads expand chunk k's compact
     * records while later chunks stream. */
    HostPool *sp = ensure_stage_pool(c);
    for (uint32_t k = 0; k < std::min<uint32_t>(K, 2) && !rc; k++)
        if (!(rc = stage_host_copy(xs[k], residues, seq_offsets, cut[k], cut[k + 1], sp)))
            rc = enqueue_chunk(xs[k], params, want, c->chunk_counts[k]);
    const bool timing = std::getenv("KGX_TIMING") != nullptr;
    for (uint32_t k = 0; k < K && !rc; k++) {
        kgx_ctx *x = xs[k & 1];
        const auto t0 = now();
        HIP_TRY(hipEventSynchronize(c->chunk_counts[k])); /* chunk k's counts are on the host */
        const auto t1 = now();
        const uint32_t s0 = cut[k], n = cut[k + 1] - cut[k];
        HIP_TRY(x->h_dense_hoff.resize(n + 1));
        HIP_TRY(x->h_dense_coff.resize(n + 1));
        HIP_TRY(x->h_dense_ooff.resize(n + 1));
        uint64_t nh = 0, nc = 0, no = 0;
        for (uint32_t i = 0; i < n; i++) {
            x->h_dense_hoff[i] = nh;
            x->h_dense_coff[i] = nc;
            x->h_dense_ooff[i] = no;
            nh += x->h_hcount[i];
            nc += want_calls ? x->h_ccount[i] : 0;
            no += want_otu ? x->h_ocount[i] : 0;
            c->h_hoff[s0 + i + 1] = hbase + nh;
            c->h_coff[s0 + i + 1] = cbase + nc;
            c->h_ooff[s0 + i + 1] = obase + no;
        }
        x->h_dense_hoff[n] = nh;
        x->h_dense_coff[n] = nc;
        x->h_dense_ooff[n] = no;
        nwin += x->h_nwin[0];
        const uint64_t nh_all = nh; /* hit offsets count every hit; records only when wanted */
        if (!need_hits)
            nh = 0;
        const uint64_t hrec = need_hits ? hbase : 0; /* where this chunk's records go */
        const uint64_t nwords = compact && nh ? (x->h_nwin[0] + 63) / 64 : 0;
        if (hrec + nh > c->h_hits.cap || cbase + nc > c->h_calls.cap || obase + no > c->h_otus.cap ||
            (compact && (hrec + nh > c->h_hits16.cap || mbase + nwords > c->h_mask.cap))) {
            /* growth moves the pinned arrays: no copy into them may be in
             * flight, and no expansion may be reading or writing them */
            HIP_TRY(hipStreamSynchronize(cs));
            if (compact && (rc = c->pool->wait()))
                break;
        }
        if (compact) {
            HIP_TRY(c->h_hits16.resize(hrec + nh));
            HIP_TRY(c->h_mask.resize(mbase + nwords));
        }
        if (!(compact && c->compact_out))
            HIP_TRY(c->h_hits.resize(hrec + nh));
        HIP_TRY(c->h_calls.resize(cbase + nc));
        HIP_TRY(c->h_otus.resize(obase + no));
        /* x's dense buffers still feed chunk k-2's bulk copy */
        if (k >= 2)
            HIP_TRY(hipStreamWaitEvent(x->stream, c->chunk_done[k - 2], 0));
        if (nh || nc || no) {
            HIP_TRY(x->dense_hoff.reserve((n + 1) * sizeof(uint64_t)));
            HIP_TRY(x->dense_coff.reserve((n + 1) * sizeof(uint64_t)));
            HIP_TRY(x->dense_ooff.reserve((n + 1) * sizeof(uint64_t)));
            HIP_TRY(x->dense_hits.reserve(std::max<uint64_t>(nh, 1) * sizeof(kgx_hit)));
            HIP_TRY(x->dense_calls.reserve(std::max<uint64_t>(nc, 1) * sizeof(kgx_call)));
            HIP_TRY(x->dense_otus.reserve(std::max<uint64_t>(no, 1) * sizeof(kgx_otu)));
            HIP_TRY(hipMemcpyAsync(x->dense_hoff.p, x->h_dense_hoff.data(), (n + 1) * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, x->stream));
            HIP_TRY(hipMemcpyAsync(x->dense_coff.p, x->h_dense_coff.data(), (n + 1) * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, x->stream));
            HIP_TRY(hipMemcpyAsync(x->dense_ooff.p, x->h_dense_ooff.data(), (n + 1) * sizeof(uint64_t),
                                   hipMemcpyHostToDevice, x->stream));
            HIP_TRY(launch_gather(n, x->wbase.as<uint64_t>(), x->hit_mask.as<uint64_t>(), x->tile_windows,
                                  x->call_count.as<uint32_t>(), x->hits.as<uint4>(),
                                  x->hits.as<uint4>() + x->hit_slots, x->calls.as<kgx_call>(),
                                  x->dense_hoff.as<uint64_t>(), x->dense_coff.as<uint64_t>(),
                                  nh && !compact ? x->dense_hits.as<kgx_hit>() : nullptr,
                                  nc ? x->dense_calls.as<kgx_call>() : nullptr, s0, x->hit_format,
                                  x->otu_count.as<uint32_t>(), x->otus.as<kgx_otu>(), x->dense_ooff.as<uint64_t>(),
                                  no ? x->dense_otus.as<kgx_otu>() : nullptr, x->stream,
                                  nh && compact ? x->dense_hits.as<uint4>() : nullptr));
        }
        /* the mask and best calls too: chunk k+2's kernels overwrite them */
        if ((rc = keep_mask(x, nwords)) || (want_best && (rc = keep_best(x, n))))
            break;
        HIP_TRY(hipEventRecord(c->chunk_gathered[k], x->stream));
        HIP_TRY(hipStreamWaitEvent(cs, c->chunk_gathered[k], 0));
        if (k + 1 < K && c->opt.counts_first)
            HIP_TRY(hipStreamWaitEvent(cs, c->chunk_counts[k + 1], 0));
        if (compact) {
            if ((rc = copy_out(c->h_hits16, hrec, x->dense_hits.p, nh)) ||
                (rc = copy_out(c->h_mask, mbase, x->dense_mask.p, nwords)))
                break;
        } else if ((rc = copy_out(c->h_hits, hrec, x->dense_hits.p, nh))) {
            break;
        }
        if ((rc = copy_out(c->h_calls, cbase, x->dense_calls.p, nc)) ||
            (rc = copy_out(c->h_otus, obase, x->dense_otus.p, no)) ||
            (want_best && (rc = copy_out(c->h_best, s0, x->dense_best.p, n))))
            break;
        HIP_TRY(hipEventRecord(c->chunk_done[k], cs));
        if (compact && nh && c->compact_out) {
            /* compact results: the records stay where they land */
            c->compact_segs.push_back({s0, s0 + n, 4u, hbase, hrec, mbase});
        } else if (compact && nh) {
            /* host threads expand this chunk once its bytes have landed */
            submit_expansion(c, false, residues, seq_offsets, k, s0, n, mbase, 0, c->chunk_done[k], nullptr);
        }
        mbase += nwords;
        hbase += nh_all;
        cbase += nc;
        obase += no;
        const auto t2 = now();
        /* chunk k+2 -> x (its H2D of chunk k finished before chunk k's counts
         * arrived), enqueued at once */
        if (k + 2 < K && !(rc = stage_host_copy(x, residues, seq_offsets, cut[k + 2], cut[k + 3], sp)))
            rc = enqueue_chunk(x, params, want, c->chunk_counts[k + 2]);
        if (timing)
            std::fprintf(stderr, "[kgx] chunk %u: wait counts %.3f ms, enqueue %.3f ms, stage+enqueue k+2 %.3f ms\n",
                         k, ms(t0, t1), ms(t1, t2), ms(t2, now()));
    }
    /* drain both streams, whatever happened above */
    const hipError_t e0 = hipStreamSynchronize(xs[0]->stream), e1 = hipStreamSynchronize(xs[1]->stream);
    const hipError_t e2 = hipStreamSynchronize(cs);
    const int prc = compact ? c->pool->wait() : KGX_OK;
    if (rc)
        return rc;
    if (prc)
        return prc;
    HIP_TRY(e0);
    HIP_TRY(e1);
    HIP_TRY(e2);
    /* the batch's device results are split over two contexts */
    c->have_hits = false;
    t->have_hits = false;
    fill_result(c, n_seq, need_hits, (want & KGX_WANT_BEST) != 0, nwin, out);
    return KGX_OK;
}

inline uint64_t round16(uint64_t bytes) { return (bytes + 15) & ~15ull; }

/* whether a host batch can take the one-launch path (kgx_fused.hip) */
bool fused_eligible(const kgx_ctx *c, const kgx_params &p, const uint64_t *seq_offsets, uint32_t n_seq,
                    uint32_t want)
{
    if (!c->opt.small_fused || c->img->layout != KGX_LAYOUT_PACKED16 || !c->img->d_packed || n_seq == 0 ||
        n_seq > FUSED_MAX_SEQ || want == 0 || (want & ~(KGX_WANT_HITS | KGX_WANT_CALLS)) || p.order_constraint != 0 ||
        p.min_hits < 1)
        return false;
    for (uint32_t s = 0; s < n_seq; s++)
        if (windows_of(seq_offsets[s + 1] - seq_offsets[s]) > FUSED_MAX_WINDOWS)
            return false;
    return true;
}

/* A small host batch in ONE launch: one workgroup per sequence reads its
 * residues from the pinned staging, probes, compacts, scores and stores its
 * kgx_hit / kgx_call records into per-sequence regions of mapped memory
 * (from the sequence's first window), then its count and a completion
 * token; the host polls the tokens and packs the regions into the CSR
 * result.  The device keeps no batch (kgx_kmap_add_hits needs another path:
 * the option is for per-sequence callers, e.g. the facade's process_aa_seq). */
int process_batch_fused(kgx_ctx *c, const kgx_params &p, const char *residues, const uint64_t *seq_offsets,
                        uint32_t n_seq, uint32_t want, kgx_result *out)
{
    int rc = stage_host_copy(c, residues, seq_offsets, 0, n_seq);
    if (rc)
        return rc;
    const uint64_t *off = c->h_off_stage.data();
    HIP_TRY(c->h_fwb.resize(n_seq + 1));
    uint64_t W = 0, longest = 0;
    for (uint32_t s = 0; s < n_seq; s++) {
        c->h_fwb[s] = W;
        const uint64_t w = windows_of(off[s + 1] - off[s]);
        W += w;
        longest = std::max(longest, w);
    }
    c->h_fwb[n_seq] = W;
    const bool need_hits = (want & KGX_WANT_HITS) != 0, want_calls = (want & KGX_WANT_CALLS) != 0;
    HIP_TRY(c->h_fhits.resize(std::max<uint64_t>(W, 1)));
    HIP_TRY(c->h_fcalls.resize(std::max<uint64_t>(W, 1)));
    HIP_TRY(c->h_fcounts.resize(2 * (uint64_t)n_seq));
    HIP_TRY(c->h_fdone.resize(n_seq));
    HIP_TRY(c->h_res.resize(std::max<uint64_t>(c->h_res.size(), 1)));
    void *d_res = nullptr, *d_off = nullptr, *d_wb = nullptr, *d_hits = nullptr, *d_calls = nullptr,
         *d_counts = nullptr, *d_done = nullptr;
    HIP_TRY(c->h_res.device_ptr(0, &d_res));
    HIP_TRY(c->h_off_stage.device_ptr(0, &d_off));
    HIP_TRY(c->h_fwb.device_ptr(0, &d_wb));
    HIP_TRY(c->h_fhits.device_ptr(0, &d_hits));
    HIP_TRY(c->h_fcalls.device_ptr(0, &d_calls));
    HIP_TRY(c->h_fcounts.device_ptr(0, &d_counts));
    HIP_TRY(c->h_fdone.device_ptr(0, &d_done));
    const uint32_t token = ++c->small_token ? c->small_token : ++c->small_token;
    /* KGX_FUSED_DEBUG: wall-clock stamps of the first workgroup's phases, to stderr */
    static const bool debug = std::getenv("KGX_FUSED_DEBUG") != nullptr;
    void *d_dbg = nullptr;
    if (debug) {
        HIP_TRY(c->h_fdbg.resize(16));
        std::memset(c->h_fdbg.data(), 0, 16 * sizeof(uint64_t));
        HIP_TRY(c->h_fdbg.device_ptr(0, &d_dbg));
    }
    HIP_TRY(launch_fused_small(static_cast<const uint8_t *>(d_res), static_cast<const uint64_t *>(d_off),
                               static_cast<const uint64_t *>(d_wb), n_seq, want, ctx_probe_table(c), p,
                               static_cast<kgx_hit *>(d_hits), static_cast<kgx_call *>(d_calls),
                               static_cast<uint32_t *>(d_counts), static_cast<uint32_t *>(d_done), token,
                               (uint32_t)longest, static_cast<uint64_t *>(d_dbg), c->h_off_stage.data(),
                               c->h_fwb.data(), reinterpret_cast<const uint8_t *>(c->h_res.data()),
                               c->opt.fused_inline && n_seq <= FUSED_INLINE_SEQ && off[n_seq] <= FUSED_INLINE_RES
                                   ? (uint32_t)std::max<uint64_t>(off[n_seq], 1)
                                   : 0u,
                               c->stream));
    /* every sequence's token (stored after its results, behind a
     * system-scope fence); a fault or a lost store still ends the wait */
    const volatile uint32_t *done = c->h_fdone.data();
    for (uint32_t s = 0; s < n_seq; s++)
        for (uint32_t spin = 1; done[s] != token; spin++) {
            if ((spin & 255u) == 0) {
                const hipError_t q = hipStreamQuery(c->stream);
                if (q == hipSuccess) {
                    std::atomic_thread_fence(std::memory_order_acquire);
                    if (done[s] != token)
                        return fail(KGX_EDEVICE, "fused batch: sequence " + std::to_string(s) +
                                                     " ended without its completion token");
                    break;
                }
                if (q != hipErrorNotReady)
                    HIP_TRY(q);
            }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
        }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (debug) {
        const uint64_t *d = c->h_fdbg.data();
        std::fprintf(stderr, "[kgx] fused n=%u: load %llu, probe %llu, compact %llu, store+score %llu, fence %llu ticks\n",
                     n_seq, (unsigned long long)(d[1] - d[0]), (unsigned long long)(d[2] - d[1]),
                     (unsigned long long)(d[3] - d[2]), (unsigned long long)(d[4] - d[3]),
                     (unsigned long long)(d[5] - d[4]));
    }
    /* the regions -> the CSR result */
    const uint32_t *cnt = c->h_fcounts.data();
    c->h_hoff.assign(n_seq + 1, 0);
    c->h_coff.assign(n_seq + 1, 0);
    c->h_ooff.assign(n_seq + 1, 0);
    for (uint32_t s = 0; s < n_seq; s++) {
        const uint64_t w = c->h_fwb[s + 1] - c->h_fwb[s];
        if (cnt[s] > w || cnt[n_seq + s] > w)
            return fail(KGX_EDEVICE, "fused batch: more records than windows");
        c->h_hoff[s + 1] = c->h_hoff[s] + cnt[s];
        c->h_coff[s + 1] = c->h_coff[s] + (want_calls ? cnt[n_seq + s] : 0u);
    }
    HIP_TRY(c->h_hits.resize(need_hits ? c->h_hoff[n_seq] : 0));
    HIP_TRY(c->h_calls.resize(c->h_coff[n_seq]));
    HIP_TRY(c->h_otus.resize(0));
    for (uint32_t s = 0; s < n_seq; s++) {
        if (need_hits && cnt[s])
            std::memcpy(c->h_hits.data() + c->h_hoff[s], c->h_fhits.data() + c->h_fwb[s], cnt[s] * sizeof(kgx_hit));
        if (want_calls && cnt[n_seq + s])
            std::memcpy(c->h_calls.data() + c->h_coff[s], c->h_fcalls.data() + c->h_fwb[s],
                        cnt[n_seq + s] * sizeof(kgx_call));
    }
    c->have_hits = false; /* nothing of the batch stays on the device */
    c->have_best = false;
    c->have_otus = false;
    fill_result(c, n_seq, need_hits, false, W, out);
    return KGX_OK;
}

/* A small host batch (process_aa_seq's one sequence, a request's few) in one
 * host wait: the host writes the plan (window bases, tile owners, longest
 * sequence) beside the staged residues and offsets in one pinned blob, one
 * kernel pulls the blob into the plan's buffers, the probe and scorer run as
 * for any batch, and one workgroup scans the counts into the CSR offsets, which
 * the gather uses to store the records straight into mapped result arrays
 * sized for the worst case (every window a hit).  Same kernels, same records
 * as kgx_run_device + kgx_device_batch_collect. */
int process_batch_small(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                        uint32_t n_seq, uint32_t want, kgx_result *out, kgx_kmap *roll_map = nullptr,
                        int roll_mode = 0)
{
    PhaseTimer tm(c); /* KGX_TIMING: phase times (each mark waits for the stream) */
    int rc = stage_host_copy(c, residues, seq_offsets, 0, n_seq);
    if (rc)
        return rc;
    tm.mark("s.stage");
    const uint64_t n_res = c->h_res.size();
    const uint64_t *off = c->h_off_stage.data();
    HIP_TRY(c->residues.reserve(round16(n_res + 16)));
    HIP_TRY(c->offsets.reserve(round16((n_seq + 1) * sizeof(uint64_t))));
    if ((rc = plan_reserve(c, c->offsets.as<uint64_t>(), n_seq, n_res)))
        return rc;
    HIP_TRY(c->wbase.reserve(round16((n_seq + 1) * sizeof(uint64_t))));
    HIP_TRY(c->tile_seq.reserve(round16(c->max_tiles * sizeof(uint32_t))));
    /* the blob: offsets | window bases | tile owners | status | residues */
    const uint64_t b_off = round16((n_seq + 1) * sizeof(uint64_t)), b_wb = b_off,
                   b_tile = round16(c->max_tiles * sizeof(uint32_t)), b_st = 16, b_res = round16(n_res);
    /* the residues stay in the pinned staging (h_res): the upload reads them
     * from there, no second host copy */
    const uint64_t words = (b_off + b_wb + b_tile + b_st) / 16;
    HIP_TRY(c->h_small.resize(words));
    HIP_TRY(c->h_res.resize(b_res ? b_res : 16)); /* 16-B words: the upload's last one may run past n_res */
    char *blob = reinterpret_cast<char *>(c->h_small.data());
    uint64_t *h_off = reinterpret_cast<uint64_t *>(blob);
    uint64_t *h_wb = reinterpret_cast<uint64_t *>(blob + b_off);
    uint32_t *h_tile = reinterpret_cast<uint32_t *>(blob + b_off + b_wb);
    uint32_t *h_st = reinterpret_cast<uint32_t *>(blob + b_off + b_wb + b_tile);
    std::memcpy(h_off, off, (n_seq + 1) * sizeof(uint64_t));
    /* plan_reduce / plan_scan on the host: window bases, the sequence owning
     * each tile's first window, the longest sequence */
    const uint64_t T = c->tile_windows;
    uint64_t wb = 0;
    uint32_t longest = 0;
    for (uint32_t s = 0; s < n_seq; s++) {
        const uint64_t w = windows_of(off[s + 1] - off[s]);
        h_wb[s] = wb;
        for (uint64_t t = (wb + T - 1) / T; t * T < wb + w; t++)
            h_tile[t] = s;
        wb += w;
        longest = (uint32_t)std::max<uint64_t>(longest, std::min<uint64_t>(w, 0xFFFFFFFFull));
    }
    h_wb[n_seq] = wb;
    for (uint64_t t = (wb + T - 1) / T; t < c->max_tiles; t++)
        h_tile[t] = n_seq ? n_seq - 1 : 0; /* tiles past the last window (never probed) */
    h_st[0] = 0;
    h_st[1] = longest;
    h_st[2] = h_st[3] = 0;
    void *d_blob = nullptr, *d_res = nullptr;
    HIP_TRY(c->h_small.device_ptr(0, &d_blob));
    HIP_TRY(c->h_res.device_ptr(0, &d_res));
    const uint4 *src = static_cast<const uint4 *>(d_blob);
    SmallPieces pc;
    const uint64_t sizes[SMALL_PIECES] = {b_off, b_wb, b_tile, b_st, b_res};
    void *dsts[SMALL_PIECES] = {c->offsets.p, c->wbase.p, c->tile_seq.p, c->plan_status.p, c->residues.p};
    uint64_t at = 0;
    for (int p = 0; p < SMALL_PIECES; p++) {
        pc.dst[p] = static_cast<uint4 *>(dsts[p]);
        /* the last piece (residues) from the staging, the others from the blob */
        pc.src[p] = p == SMALL_PIECES - 1 ? static_cast<const uint4 *>(d_res) : src + at;
        at += sizes[p] / 16;
        pc.end16[p] = at;
    }
    tm.mark("s.plan");
    HIP_TRY(launch_small_upload(pc, c->stream));
    tm.mark("s.upload");
    /* a small probe neither waits for nor holds back the image's other probes:
     * chaining it (probe_serialize, for probes that fill the chip) would make
     * the pool's per-sequence calls run one at a time across worker threads */
    const int serialize = c->opt.probe_serialize;
    c->opt.probe_serialize = 0;
    rc = kgx_stage_probe(c, c->residues.as<uint8_t>(), c->offsets.as<uint64_t>());
    c->opt.probe_serialize = serialize;
    if (rc)
        return rc;
    tm.mark("s.probe");
    /* the scorer: with few sequences the lane machine's one-lane chain per
     * sequence is the whole stage's latency (31 us for one 300-aa protein);
     * the wave scorer spreads each sequence's hits over a wave (option
     * small_wave; the lane machine still takes order_constraint 1) */
    const int variant = c->opt.score_variant, wave_tiles = c->opt.score_wave_tiles;
    if (c->opt.small_wave && variant == SCORE_HYBRID) /* the host plan knows the longest sequence */
        c->opt.score_variant = longest <= (uint32_t)RUN_CAP ? SCORE_WAVE_ONLY : SCORE_WAVE;
    /* a wave walks the sequences that start in its tiles one after another:
     * few tiles per wave (option small_wave_tiles) put a coalesced batch's
     * sequences on different waves, scored at once */
    c->opt.score_wave_tiles = c->opt.small_wave_tiles;
    /* past SMALL_GATHER_SEQ sequences the collect decides the best calls */
    const bool collect_best = (want & KGX_WANT_BEST) && n_seq > SMALL_GATHER_SEQ && n_seq <= SMALL_COLLECT_BEST_SEQ;
    c->defer_best = collect_best;
    rc = kgx_stage_score(c, params, want);
    c->defer_best = false;
    c->opt.score_variant = variant;
    c->opt.score_wave_tiles = wave_tiles;
    tm.mark("s.score");
    if (rc)
        return rc;
    /* results: worst-case mapped arrays, offsets and totals in mapped memory */
    const bool want_calls = (want & KGX_WANT_CALLS) != 0, want_otu = (want & KGX_WANT_OTU) != 0,
               need_hits = (want & KGX_WANT_HITS) != 0, want_best = (want & KGX_WANT_BEST) != 0;
    const uint64_t cap = std::max<uint64_t>(wb, 1);
    HIP_TRY(c->dense_hoff.reserve((n_seq + 1) * sizeof(uint64_t)));
    HIP_TRY(c->dense_coff.reserve((n_seq + 1) * sizeof(uint64_t)));
    HIP_TRY(c->dense_ooff.reserve((n_seq + 1) * sizeof(uint64_t)));
    HIP_TRY(c->h_dense_hoff.resize(n_seq + 1));
    HIP_TRY(c->h_dense_coff.resize(n_seq + 1));
    HIP_TRY(c->h_dense_ooff.resize(n_seq + 1));
    HIP_TRY(c->h_plan_status.resize(1));
    HIP_TRY(c->h_nwin.resize(1));
    HIP_TRY(c->h_hits.resize(need_hits ? cap : 0));
    HIP_TRY(c->h_calls.resize(want_calls ? cap : 0));
    HIP_TRY(c->h_otus.resize(want_otu ? cap : 0));
    HIP_TRY(c->h_best.resize(want_best ? n_seq : 0));
    void *m_hoff, *m_coff, *m_ooff, *m_st, *m_nwin, *mh = nullptr, *mc = nullptr, *mo = nullptr, *mb = nullptr;
    HIP_TRY(c->h_dense_hoff.device_ptr(0, &m_hoff));
    HIP_TRY(c->h_dense_coff.device_ptr(0, &m_coff));
    HIP_TRY(c->h_dense_ooff.device_ptr(0, &m_ooff));
    HIP_TRY(c->h_plan_status.device_ptr(0, &m_st));
    HIP_TRY(c->h_nwin.device_ptr(0, &m_nwin));
    if (need_hits)
        HIP_TRY(c->h_hits.device_ptr(0, &mh));
    if (want_calls)
        HIP_TRY(c->h_calls.device_ptr(0, &mc));
    if (want_otu)
        HIP_TRY(c->h_otus.device_ptr(0, &mo));
    if (want_best && n_seq)
        HIP_TRY(c->h_best.device_ptr(0, &mb));
    /* the fused gather stores a fresh token last; the host polls it (a stream
     * sync costs several us more than the kernel's own end) */
    const bool fused = n_seq <= SMALL_GATHER_SEQ;
    const uint32_t token = ++c->small_token ? c->small_token : ++c->small_token;
    void *m_done = nullptr;
    if (fused) {
        HIP_TRY(c->h_done.resize(1));
        c->h_done[0] = 0;
        HIP_TRY(c->h_done.device_ptr(0, &m_done));
        if (!c->small_blocks_done.p) { /* the gather's workgroup counter, zero between launches */
            HIP_TRY(c->small_blocks_done.reserve(sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(c->small_blocks_done.p, 0, sizeof(uint32_t), c->stream));
        }
    }
    if (fused) { /* scan + gather in one workgroup */
        HIP_TRY(launch_small_gather(n_seq, c->wbase.as<uint64_t>(), c->hit_mask.as<uint64_t>(), c->tile_windows,
                                    c->hit_count.as<uint32_t>(), c->call_count.as<uint32_t>(), c->hits.as<uint4>(),
                                    c->hits.as<uint4>() + c->hit_slots, c->calls.as<kgx_call>(),
                                    c->otu_count.as<uint32_t>(), c->otus.as<kgx_otu>(), static_cast<kgx_hit *>(mh),
                                    static_cast<kgx_call *>(mc), static_cast<kgx_otu *>(mo),
                                    static_cast<uint64_t *>(m_hoff), static_cast<uint64_t *>(m_coff),
                                    static_cast<uint64_t *>(m_ooff), c->plan_status.as<uint32_t>(),
                                    want_best ? c->best.as<kgx_best_call>() : nullptr,
                                    static_cast<kgx_best_call *>(mb), static_cast<uint32_t *>(m_st),
                                    static_cast<uint64_t *>(m_nwin), static_cast<uint32_t *>(m_done), token,
                                    c->small_blocks_done.as<uint32_t>(), c->hit_format, c->stream));
    } else if (collect_best) {
        HIP_TRY(launch_small_collect_best(
            n_seq, c->hit_count.as<uint32_t>(), want_calls ? c->call_count.as<uint32_t>() : nullptr,
            want_otu ? c->otu_count.as<uint32_t>() : nullptr, c->dense_hoff.as<uint64_t>(),
            c->dense_coff.as<uint64_t>(), c->dense_ooff.as<uint64_t>(), static_cast<uint64_t *>(m_hoff),
            static_cast<uint64_t *>(m_coff), static_cast<uint64_t *>(m_ooff), c->plan_status.as<uint32_t>(),
            c->wbase.as<uint64_t>(), c->calls.as<kgx_call>(), c->call_count.as<uint32_t>(),
            c->best_ws.as<kgx_call>(), c->best.as<kgx_best_call>(), static_cast<kgx_best_call *>(mb),
            static_cast<uint32_t *>(m_st), static_cast<uint64_t *>(m_nwin), c->stream));
    } else {
        HIP_TRY(launch_small_collect(n_seq, c->hit_count.as<uint32_t>(),
                                     want_calls ? c->call_count.as<uint32_t>() : nullptr, want_otu ? c->otu_count.as<uint32_t>() : nullptr, c->dense_hoff.as<uint64_t>(),
                                     c->dense_coff.as<uint64_t>(), c->dense_ooff.as<uint64_t>(),
                                     static_cast<uint64_t *>(m_hoff), static_cast<uint64_t *>(m_coff),
                                     static_cast<uint64_t *>(m_ooff), c->plan_status.as<uint32_t>(),
                                     c->wbase.as<uint64_t>(), want_best ? c->best.as<kgx_best_call>() : nullptr,
                                     static_cast<kgx_best_call *>(mb), static_cast<uint32_t *>(m_st),
                                     static_cast<uint64_t *>(m_nwin), c->stream));
    }
    if (!fused && (mh || mc || mo)) /* a counts-and-best-calls batch (/lookup's) gathers nothing */
        HIP_TRY(launch_gather(n_seq, c->wbase.as<uint64_t>(), c->hit_mask.as<uint64_t>(), c->tile_windows,
                              c->call_count.as<uint32_t>(), c->hits.as<uint4>(),
                              c->hits.as<uint4>() + c->hit_slots, c->calls.as<kgx_call>(),
                              c->dense_hoff.as<uint64_t>(), c->dense_coff.as<uint64_t>(),
                              static_cast<kgx_hit *>(mh), static_cast<kgx_call *>(mc), 0u, c->hit_format,
                              c->otu_count.as<uint32_t>(), c->otus.as<kgx_otu>(), c->dense_ooff.as<uint64_t>(),
                              static_cast<kgx_otu *>(mo), c->stream));
    /* kgx_lookup: the rollup queued behind the pass, one host wait for both */
    if (roll_map) {
        if ((rc = rollup_enqueue(roll_map, c, roll_mode)))
            return rc;
        HIP_TRY(host_wait(c->stream));
    }
    if (fused) {
        const volatile uint32_t *done = c->h_done.data();
        HIP_TRY(host_wait_word(done, token, c->stream));
        std::atomic_thread_fence(std::memory_order_acquire);
        /* the stream drained without the gather's last store: its results
         * are not there (an early exit or a lost store), never hand them out */
        if (*done != token)
            return fail(KGX_EDEVICE, "small batch: the gather ended without its completion token");
    } else {
        HIP_TRY(host_wait(c->stream));
    }
    if (c->h_plan_status[0])
        return fail(KGX_EINVAL, "small batch: plan status raised");
    c->h_hoff.assign(c->h_dense_hoff.data(), c->h_dense_hoff.data() + n_seq + 1);
    c->h_coff.assign(c->h_dense_coff.data(), c->h_dense_coff.data() + n_seq + 1);
    c->h_ooff.assign(c->h_dense_ooff.data(), c->h_dense_ooff.data() + n_seq + 1);
    const uint64_t nh = c->h_hoff[n_seq], nc = c->h_coff[n_seq], no = c->h_ooff[n_seq];
    if ((need_hits && nh > cap) || (want_calls && nc > cap) || (want_otu && no > cap))
        return fail(KGX_EDEVICE, "small batch: more records than windows");
    HIP_TRY(c->h_hits.resize(need_hits ? nh : 0));
    HIP_TRY(c->h_calls.resize(nc));
    HIP_TRY(c->h_otus.resize(no));
    tm.mark("s.gather");
    fill_result(c, n_seq, need_hits, want_best, c->h_nwin[0], out);
    return KGX_OK;
}

/* One pass over the whole host batch (its results stay on the device for
 * kgx_kmap_rollup / kgx_kmap_add_hits / kgx_matrix_add_hits).  Residues in
 * the caller's pinned memory go up by DMA straight from there (option
 * "pinned_input"; a NUL among them reruns the batch staged, cut at the NUL);
 * others are staged into pinned memory on the stage pool's threads. */
int process_batch_one_pass(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                           uint32_t n_seq, uint32_t want, kgx_result *out)
{
    PhaseTimer tm(c);
    int rc = one_pass_enqueue(c, params, residues, seq_offsets, n_seq, want, nullptr, nullptr);
    if (rc)
        return rc;
    tm.mark("enqueue");
    rc = one_pass_collect(c, params, residues, seq_offsets, n_seq, want, out);
    tm.mark("collect");
    return rc;
}

/* into how many chunks a host batch goes: each at least 2M residues and one sequence */
uint32_t host_chunk_count(const kgx_ctx *c, uint64_t n_res, uint32_t n_seq)
{
    const uint64_t k_res = std::max<uint64_t>(1, n_res >> 21);
    return (uint32_t)std::min<uint64_t>({(uint64_t)c->opt.host_chunks, k_res, (uint64_t)n_seq});
}

kgx_params params_or_default(const kgx_params *params)
{
    kgx_params p;
    if (params)
        p = *params;
    else
        kgx_params_default(&p);
    return p;
}

}  // namespace

int kgx_process_batch(kgx_ctx *c, const kgx_params *params, const char *residues,
                      const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_result *out)
{
    if (!c || !out || (!seq_offsets && n_seq))
        return fail(KGX_EINVAL, "null argument");
    const uint64_t r0 = n_seq ? seq_offsets[0] : 0;
    const uint64_t n_res = n_seq ? seq_offsets[n_seq] - r0 : 0;
    for (uint32_t s = 0; s < n_seq; s++)
        if (seq_offsets[s + 1] < seq_offsets[s])
            return fail(KGX_EINVAL, "seq_offsets not monotone");
    if (n_res && !residues)
        return fail(KGX_EINVAL, "null residues");
    HIP_TRY(hipSetDevice(c->img->device));
    /* chunks only when there is something to copy back */
    const uint32_t K = host_chunk_count(c, n_res, n_seq);
    if (K >= 2 && (want & (KGX_WANT_HITS | KGX_WANT_CALLS | KGX_WANT_OTU | KGX_WANT_BEST)))
        return process_batch_chunked(c, params, residues, seq_offsets, n_seq, want, K, out);
    if (n_seq && n_res <= (uint64_t)c->opt.small_batch && n_seq <= (1u << 16)) {
        const kgx_params p = params_or_default(params);
        if (fused_eligible(c, p, seq_offsets, n_seq, want)) {
            c->fused_batches++;
            return process_batch_fused(c, p, residues, seq_offsets, n_seq, want, out);
        }
        c->small_batches++;
        return process_batch_small(c, params, residues, seq_offsets, n_seq, want, out);
    }
    return process_batch_one_pass(c, params, residues, seq_offsets, n_seq, want, out);
}

extern "C++" {
namespace kgx {

/* kgx_lookup over a batch kgx_process_batch would take down the small-batch
 * path: that path with the rollup queued behind the pass and one host wait
 * for both (*taken = true); other batches are left to the caller */
int lookup_small(kgx_ctx *c, kgx_kmap *m, int mode, const kgx_params *params, const char *residues,
                 const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_result *out, bool *taken)
{
    *taken = false;
    const uint64_t n_res = n_seq ? seq_offsets[n_seq] - seq_offsets[0] : 0;
    if (!n_seq || n_res > (uint64_t)c->opt.small_batch || n_seq > (1u << 16) || (n_res && !residues))
        return KGX_OK;
    if (host_chunk_count(c, n_res, n_seq) >= 2)
        return KGX_OK;
    if (fused_eligible(c, params_or_default(params), seq_offsets, n_seq, want))
        return KGX_OK; /* the fused kernel keeps nothing on the device to roll up */
    HIP_TRY(hipSetDevice(c->img->device));
    *taken = true;
    c->small_batches++;
    return process_batch_small(c, params, residues, seq_offsets, n_seq, want, out, m, mode);
}

}  // namespace kgx
}  // extern "C++"

int kgx_process_batch_compact(kgx_ctx *c, const kgx_params *params, const char *residues,
                              const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_compact_result *out)
{
    if (!c || !out)
        return fail(KGX_EINVAL, "null argument");
    c->compact_segs.clear();
    c->compact_chunks.clear();
    c->compact_out = 1;
    const int rc = kgx_process_batch(c, params, residues, seq_offsets, n_seq, want, &out->r);
    c->compact_out = 0;
    out->n_chunks = 0;
    out->chunks = nullptr;
    if (rc) {
        c->compact_segs.clear();
        return rc;
    }
    if (!c->compact_segs.empty()) {
        /* the pinned arrays no longer move: offsets -> pointers */
        for (const auto &g : c->compact_segs) {
            kgx_hit_chunk ch{};
            ch.seq_begin = g.s0;
            ch.seq_end = g.s1;
            ch.record_words = g.words;
            ch.hit_begin = g.hit_begin;
            ch.records = g.words == 3 ? c->h_hits12.data() + 3 * g.rec_at
                                      : reinterpret_cast<const uint32_t *>(c->h_hits16.data() + g.rec_at);
            ch.mask = c->h_mask.data() + g.mask_at;
            ch.window_start = c->h_wstart.data() + g.s0;
            c->compact_chunks.push_back(ch);
        }
        out->r.hits = nullptr;
        out->n_chunks = (uint32_t)c->compact_chunks.size();
        out->chunks = c->compact_chunks.data();
    }
    return KGX_OK;
}

int kgx_compact_expand(const kgx_compact_result *r, const char *residues, const uint64_t *seq_offsets,
                       uint32_t s_begin, uint32_t s_end, uint32_t seq_base, kgx_hit *out)
{
    return compact_expand(r, residues, seq_offsets, s_begin, s_end, seq_base, out, false);
}

}  // extern "C"

int kgx::compact_expand(const kgx_compact_result *r, const char *residues, const uint64_t *seq_offsets,
                        uint32_t s_begin, uint32_t s_end, uint32_t seq_base, kgx_hit *out, bool nt)
{
    if (!r || s_begin > s_end || s_end > r->r.n_seq || !r->r.hit_offsets)
        return fail(KGX_EINVAL, "bad compact range");
    const uint64_t *hoff = r->r.hit_offsets;
    const uint64_t j0 = hoff[s_begin], j1 = hoff[s_end];
    if (j0 == j1)
        return KGX_OK;
    if (!out)
        return fail(KGX_EINVAL, "null output");
    if (r->n_chunks == 0) {
        if (!r->r.hits)
            return fail(KGX_EINVAL, "the result holds no hits (want without KGX_WANT_HITS)");
        std::memcpy(out, r->r.hits + j0, (j1 - j0) * sizeof(kgx_hit));
        if (seq_base)
            for (uint64_t j = 0; j < j1 - j0; j++)
                out[j].seq += seq_base;
        return KGX_OK;
    }
    if (!residues || !seq_offsets)
        return fail(KGX_EINVAL, "compact hits need the batch's residues and offsets");
    /* the chunks are in sequence order: the first one that ends past s_begin */
    const kgx_hit_chunk *ch = r->chunks, *end = r->chunks + r->n_chunks;
    ch = std::upper_bound(ch, end, s_begin, [](uint32_t s, const kgx_hit_chunk &x) { return s < x.seq_end; });
    uint32_t s = s_begin;
    for (; ch != end && s < s_end; ch++) {
        if (ch->seq_begin > s) {
            /* sequences between chunks have no hits (a chunk without hits has no records) */
            for (; s < std::min(ch->seq_begin, s_end); s++)
                if (hoff[s + 1] != hoff[s])
                    return fail(KGX_EINVAL, "compact hits: a sequence with hits outside every chunk");
            if (s >= s_end)
                break;
        }
        const uint32_t b = std::min(ch->seq_end, s_end);
        const int rc = expand_chunk(*ch, hoff, residues, seq_offsets, s, b, out, j0, seq_base, nt);
        if (rc)
            return rc;
        s = b;
    }
    for (; s < s_end; s++)
        if (hoff[s + 1] != hoff[s])
            return fail(KGX_EINVAL, "compact hits: a sequence with hits outside every chunk");
    return KGX_OK;
}
