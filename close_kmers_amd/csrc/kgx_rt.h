/*
 * kgx_rt.h -- host runtime internals shared by the C ABI translation units
 * (kgx_runtime.cpp: images, contexts, stages; kgx_host_batch.cpp: host-buffer
 * batches; kgx_pool.cpp: context pools; kgx_tables.hip: k-mer -> id
 * tables and /matrix pair counting).  Not part of the public ABI.
 */
#ifndef KGX_RT_H
#define KGX_RT_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kgx_internal.h"
#include "kgx_options.h"

namespace kgx {

/* sets the thread's kgx_last_error() text and returns code */
int fail(int code, const std::string &msg);
/* an on/off environment switch (KGX_LINE_HOME, KGX_LINE_MARKS, KGX_LINE_TWINS,
 * KGX_LINE_PAIRS, KGX_PROBE_DEFER): "0" clears `value`; "1", unset or empty leaves it at its
 * default; anything else is KGX_EINVAL, with `zero` and `one` naming the two
 * settings */
inline int env_switch(const char *name, const char *zero, const char *one, bool &value)
{
    const char *v = std::getenv(name);
    if (!v || !*v || !std::strcmp(v, "1"))
        return KGX_OK;
    if (std::strcmp(v, "0"))
        return fail(KGX_EINVAL, std::string(name) + ": 0 (" + zero + ") or 1 (" + one + "), not \"" + v + "\"");
    value = false;
    return KGX_OK;
}
bool is_gfx950(int dev);
/* an image from n entries that are already in HBM of `device` (keys above
 * 20^8 skipped, the lowest index of a duplicated key wins): the device half
 * of kgx_image_build */
int image_from_device_entries(int device, uint64_t num_sigs, const uint64_t *d_keys, const int32_t *d_fi,
                              const int32_t *d_otu, const uint16_t *d_avg, const float *d_wt, uint64_t n,
                              kgx_image **out, uint64_t *n_stored);

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return ::kgx::fail(KGX_EDEVICE, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

/* v holds at least n events (created with flags) */
inline int ensure_events(std::vector<hipEvent_t> &v, size_t n, unsigned flags = hipEventDisableTiming)
{
    while (v.size() < n) {
        hipEvent_t e;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        v.push_back(e);
    }
    return KGX_OK;
}

/* How a thread waits for its own stream (kgx_set_host_wait): KGX_WAIT_SPIN
 * (hipStreamSynchronize: the runtime polls), KGX_WAIT_SLEEP (hipStreamQuery
 * every poll_us, the thread asleep in between) or KGX_WAIT_BLOCK (a
 * blocking-sync event: the thread sleeps until the device signals).  A
 * server of many workers under a CPU share (the box's 16 CPUs) spends that
 * share spinning in the default; the two others hand it to the text and
 * socket work.  Process-wide; KGX_HOST_WAIT=spin|sleep[:us]|block sets the
 * starting mode. */
extern std::atomic<int> g_host_wait_mode;
extern std::atomic<uint32_t> g_host_wait_us;
hipError_t host_wait(hipStream_t s);
/* the host spins on a completion word the device stores (small batches):
 * the same modes, polling `done` instead of the stream */
hipError_t host_wait_word(const volatile uint32_t *done, uint32_t token, hipStream_t s);

/* grow-only device buffer, freed with its owner */
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap)
    {
        o.p = nullptr;
        o.cap = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(bytes, 256);
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess)
            cap = want;
        return e;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

/* grow-only pinned host array (hipHostMalloc): the staging and result
 * buffers of the host-buffer path, so H2D / D2H run at DMA speed instead of
 * through the runtime's pageable bounce buffers.  Contents are not
 * initialised on growth. */
template <class T> struct PinnedVec {
    T *p = nullptr;
    size_t n = 0, cap = 0;
    mutable void *dp = nullptr; /* p's device address, looked up once per allocation */
    PinnedVec() = default;
    PinnedVec(const PinnedVec &) = delete;
    PinnedVec &operator=(const PinnedVec &) = delete;
    ~PinnedVec()
    {
        if (p)
            (void)hipHostFree(p);
    }
    hipError_t resize(size_t m)
    {
        if (m > cap) {
            T *q = nullptr;
            const size_t want = std::max<size_t>(m + m / 4, 64);
            hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&q), want * sizeof(T), hipHostMallocDefault);
            if (e != hipSuccess)
                return e;
            if (p) {
                std::memcpy(q, p, n * sizeof(T));
                (void)hipHostFree(p);
            }
            p = q;
            cap = want;
            dp = nullptr;
        }
        n = m;
        return hipSuccess;
    }
    T *data() { return p; }
    const T *data() const { return p; }
    /* the device's address of element i (pinned host memory is mapped) */
    hipError_t device_ptr(size_t i, void **out) const
    {
        if (!dp) {
            hipError_t e = hipHostGetDevicePointer(&dp, p, 0);
            if (e != hipSuccess) {
                dp = nullptr;
                return e;
            }
        }
        *out = static_cast<char *>(dp) + i * sizeof(T);
        return hipSuccess;
    }
    size_t size() const { return n; }
    T &operator[](size_t i) { return p[i]; }
    const T &operator[](size_t i) const { return p[i]; }
};

inline uint64_t windows_of(uint64_t len) { return len >= 9 ? len - 8 : 0; }

/* [p, p + n) lies in one pinned, device-mapped host allocation (kgx_host_alloc,
 * hipHostMalloc, hipHostRegister): the device may read it by DMA directly */
bool host_pinned_range(const void *p, uint64_t n, const void **device_address = nullptr);

/* one pass over a whole host batch, split into enqueue and collect
 * (kgx_runtime.cpp): the upload by pull kernels on `up` (recording up_done)
 * when given, else on the context's stream */
class HostPool;
/* stage: the threads that copy pageable residues into the context's pinned
 * staging (null: the context's own stage pool) */
int one_pass_enqueue(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                     uint32_t n_seq, uint32_t want, hipStream_t up, hipEvent_t up_done, HostPool *stage = nullptr);
int one_pass_collect(kgx_ctx *c, const kgx_params *params, const char *residues, const uint64_t *seq_offsets,
                     uint32_t n_seq, uint32_t want, kgx_result *out);

/* host CPUs this process may keep busy: the affinity mask, capped by a
 * cgroup v2 quota (cpu.max) -- on the GPU box the mask shows the whole
 * machine while the quota is 16 */
unsigned host_cpu_budget();

/* memcpy by up to 8 host threads for large copies (host staging into pinned
 * buffers runs at several times one core's copy rate) */
inline void parallel_memcpy(void *dst, const void *src, size_t n)
{
    const size_t T = std::min<size_t>(8, n >> 23); /* one thread per 8 MiB, up to 8 */
    if (T <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; t++)
        pool.emplace_back([=]() {
            const size_t a = n * t / T, b = n * (t + 1) / T;
            std::memcpy(static_cast<char *>(dst) + a, static_cast<const char *>(src) + a, b - a);
        });
    for (auto &th : pool)
        th.join();
}

/* A few persistent host threads for work that overlaps device streams (the
 * compact host path's hit expansion).  submit() queues a task; wait() blocks
 * until every queued task has finished and returns the first nonzero code a
 * task returned (then clears it). */
class HostPool {
  public:
    explicit HostPool(unsigned n)
    {
        for (unsigned i = 0; i < n; i++)
            th_.emplace_back([this] { run(); });
    }
    HostPool(const HostPool &) = delete;
    HostPool &operator=(const HostPool &) = delete;
    ~HostPool()
    {
        {
            std::lock_guard<std::mutex> l(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto &t : th_)
            t.join();
    }
    unsigned size() const { return (unsigned)th_.size(); }
    void submit(std::function<int()> f)
    {
        {
            std::lock_guard<std::mutex> l(mu_);
            q_.push_back(std::move(f));
            pending_++;
        }
        cv_.notify_one();
    }
    int wait()
    {
        std::unique_lock<std::mutex> l(mu_);
        idle_.wait(l, [this] { return pending_ == 0; });
        const int rc = rc_;
        rc_ = 0;
        if (rc)
            fail(rc, msg_); /* the task's error text on the waiting thread */
        return rc;
    }

  private:
    void run()
    {
        for (;;) {
            std::function<int()> f;
            {
                std::unique_lock<std::mutex> l(mu_);
                cv_.wait(l, [this] { return stop_ || !q_.empty(); });
                if (q_.empty())
                    return;
                f = std::move(q_.front());
                q_.pop_front();
            }
            const int rc = f();
            const char *why = rc ? kgx_last_error() : nullptr; /* the failing thread's text */
            std::lock_guard<std::mutex> l(mu_);
            if (rc && !rc_) {
                rc_ = rc;
                msg_ = why ? why : "";
            }
            if (--pending_ == 0)
                idle_.notify_all();
        }
    }
    std::vector<std::thread> th_;
    std::deque<std::function<int()>> q_;
    std::mutex mu_;
    std::condition_variable cv_, idle_;
    size_t pending_ = 0;
    int rc_ = 0;
    std::string msg_;
    bool stop_ = false;
};

/* a fragment pass enqueued by fq_fragments_enqueue, finished by fq_fragments_finish */
struct FqPending {
    bool active = false;
    bool desc = false;
    uint32_t n_reads = 0;
    uint64_t max_frag = 0, max_res = 0;
    const uint8_t *bases = nullptr;
    uint64_t bound = 0;
};
int fq_fragments_enqueue(kgx_ctx *c, const uint8_t *d_bases, const uint64_t *d_read_off, uint32_t n_reads,
                         uint64_t n_bases, uint64_t bound);
int fq_fragments_finish(kgx_ctx *c, kgx_fragments *out);
/* n_bases: the bytes the reads span (bounds the output); bound: bytes
 * readable from d_bases (the DNA probe's limit) */
int fq_fragments(kgx_ctx *c, const uint8_t *d_bases, const uint64_t *d_read_off, uint32_t n_reads,
                 uint64_t n_bases, uint64_t bound, kgx_fragments *out);
/* kgx_fq_proteins behind its argument checks (kgx_fq.hip); the context's device is current */
int fq_proteins(kgx_ctx *c, const char *bases, const uint64_t *read_offsets, const char *ids,
                const uint64_t *id_offsets, uint32_t n_reads, kgx_fq_text *out);
/* kgx_fq_proteins_device behind its argument checks: the reads already sit
 * in c->fq_bases / fq_roff / ft_ids / ft_idoff (kgx_fq_parse_device) */
int fq_proteins_device(kgx_ctx *c, const kgx_fq_reads *reads, kgx_fq_text *out);
/* kgx_stage_probe over fragments left as DNA (launch_probe_dna) */
int stage_probe_dna(kgx_ctx *c, const uint8_t *bases, uint64_t n_bases, const uint64_t *anchors,
                    const uint64_t *d_off);
/* kgx_stage_plan's buffers and bookkeeping without the plan kernels */
int plan_reserve(kgx_ctx *c, const uint64_t *d_off, uint32_t n_seq, uint64_t n_residues);
/* whether this context's probe can take fragments as DNA */
bool probe_takes_dna(const kgx_ctx *c);
/* the lookup's plan over fragments of at least 9 residues each (every
 * fragment a fragment pass emits has >= 11): window base = residue offset - 8
 * per earlier fragment, no scan; tile owners and the longest fragment as
 * launch_plan writes them (kgx_fq.hip) */
/* kgx_inflate.hip: one wave per blocked gzip member */
hipError_t launch_inflate_members(const uint8_t *gz, const kgx_gz_member *members, uint32_t n_members, uint8_t *out,
                                  kgx_gz_status *status, kgx_inflate_stats *stats, hipStream_t stream);
hipError_t launch_fq_plan(const uint64_t *off, uint32_t n, uint64_t *wbase, uint32_t *tile_seq, uint32_t tile_windows,
                          uint32_t *status, uint32_t *block_max, hipStream_t stream);

struct SvcState;
/* stops and frees the image's call service (kgx_svc.cpp), if any */
void svc_shutdown(kgx_image *img);
/* the same, and keeps the image's service lock until the returned guard
 * goes: a call arriving meanwhile waits for it before it starts a new
 * service, so no instance is created over a table being replaced */
std::unique_lock<std::mutex> svc_shutdown_hold(kgx_image *img);
/* kgx_kmap_rollup in two steps: the device work enqueued on c's stream (no
 * host wait once an earlier rollup on c gave a size), then the wait, the size
 * check (passes 2-3 again when short) and the result */
int rollup_enqueue(kgx_kmap *m, kgx_ctx *c, int mode);
int lookup_small(kgx_ctx *c, kgx_kmap *m, int mode, const kgx_params *params, const char *residues,
                 const uint64_t *seq_offsets, uint32_t n_seq, uint32_t want, kgx_result *out, bool *taken);
/* kgx_device_batch_collect's counts (and best calls) round trip enqueued on
 * c's stream ahead of the collect, which then only waits */
int collect_counts_enqueue(kgx_ctx *c, uint32_t want);
int rollup_finish(kgx_kmap *m, kgx_ctx *c, int mode, kgx_rollup_result *out);

/* kgx_kmap_rollup's device scratch and host results (kgx_tables.hip), per
 * context: grow-only, no allocation per call once warm */
struct RollupScratch {
    DevBuf tcount, tbase, hseq, hstart, hlen, sfirst, send, ev_id, ev_w, flag, rowdata, rows2, rowcnt, rowoff, tmp;
    PinnedVec<uint64_t> h_n; /* [0] hits, [1] events, [2] rows */
    PinnedVec<uint64_t> h_off;
    PinnedVec<kgx_rollup_row> h_rows;
    uint64_t hint = 0;          /* the previous rollup's event count: the next one's size */
    uint64_t cap = 0;           /* the enqueued rollup's event capacity (0: not yet sized) */
    uint64_t presize_misses = 0;
    bool enqueued = false;
};

/* kgx_image_set_line_index (kgx_line_index.hip): an image's PACKED16 records
 * again, 4 buckets a line, each key's home at the start of its home line
 * (line_home under `home`, kgx_line_home.h) */
struct LineIndex {
    packed_bucket *records = nullptr;
    uint64_t n_lines = 0;
    uint32_t home = LINE_HOME_MOD; /* the home mode it was built with */
    bool marks = false; /* it carries overflow marks (KGX_LINE_MARKS, kgx_line_home.h) */
    bool twins = false; /* it was built with twin records (KGX_LINE_TWINS, kgx_line_home.h) */
    bool pairs = false; /* a 7-mer's two roles are homed on the halves of a 128-B block (KGX_LINE_PAIRS, kgx_line_home.h) */
    uint64_t n_twins = 0; /* how many: the keys with two home lines */
    uint32_t load = 0; /* keys per 64 lines it was built for */
    explicit operator bool() const { return records != nullptr; }
    /* what its probes take as ProbeTable.home */
    uint32_t home_word() const { return kgx::home_word(2u, home, marks, twins, pairs); }
};

}  // namespace kgx

struct kgx_image {
    int device = 0;
    uint64_t num_sigs = 0;
    int layout = KGX_LAYOUT_AOS24;
    kgx_sig_kmer *d_table = nullptr;   /* AOS24: the file's buckets */
    kgx::packed_bucket *d_packed = nullptr; /* PACKED16 */
    /* kgx_image_set_line_index: the probes read it instead of d_packed, which
     * stays for downloads, saves and filters */
    kgx::LineIndex lines;
    uint64_t *d_filter = nullptr;           /* presence filter (kgx_image_set_filter) */
    uint32_t filter_log2_words = 0;
    /* probe order across the image's contexts: the probe is bound by random
     * HBM requests, so two probes at once only share that rate; run back to
     * back instead, each context's other kernels (plan, score, gather, fq
     * translation) overlap the next context's probe */
    std::mutex probe_mu;
    hipEvent_t last_probe = nullptr; /* end of the latest probe enqueued */
    hipStream_t probe_stream = nullptr; /* contexts' chained probes with option probe_stream */
    /* the resident call service (kgx_svc.cpp), created on the first kgx_svc_call */
    std::mutex svc_mu; /* creation, configuration and shutdown; a call takes no lock */
    std::atomic<kgx::SvcState *> svc{nullptr};
    /* callers inside kgx_svc_call, counted per thread shard, each shard on a
     * line of its own: a call writes no line that other callers write
     * (kgx_svc.cpp: enter / shutdown_locked) */
    struct alignas(64) SvcUsers {
        std::atomic<uint32_t> n{0};
    };
    SvcUsers svc_users[32];
    uint32_t svc_slots = 32, svc_idle_us = 1000, svc_life_us = 1000;
    bool svc_configured = false; /* kgx_svc_config was called (env defaults no longer apply) */
    const void *resident() const
    {
        return layout == KGX_LAYOUT_PACKED16 ? static_cast<const void *>(d_packed) : d_table;
    }
    uint64_t resident_bytes() const
    {
        return num_sigs * (layout == KGX_LAYOUT_PACKED16 ? sizeof(kgx::packed_bucket) : sizeof(kgx_sig_kmer));
    }
    /* what the probes read: the line index when there is one */
    kgx::ProbeTable probe_table() const
    {
        return lines ? kgx::ProbeTable{lines.records, 4 * lines.n_lines, lines.home_word(), layout} : reference_table();
    }
    /* the resident table under the reference's slots */
    kgx::ProbeTable reference_table() const { return kgx::ProbeTable{resident(), num_sigs, 0u, layout}; }
};

struct kgx_ctx {
    kgx_image *img = nullptr;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipEvent_t probe_done = nullptr; /* recorded after each of this context's probes */
    hipEvent_t probe_ready = nullptr; /* this context's inputs are ready for its probe */
    /* a pool's /lookup: the stream the pass's score runs on after its probe
     * (null: the context's stream), behind score_gate recorded after the probe */
    hipStream_t score_stream = nullptr;
    hipEvent_t score_gate = nullptr;
    /* device scratch */
    kgx::DevBuf residues, offsets, wbase, tile_seq, hit_mask, hits, calls, hit_count, call_count,
        dense_hoff, dense_coff, dense_hits, dense_calls, plan_ws, ranges;
    /* plan status word (1 = the last plan's offsets were bad, batch emptied) */
    kgx::DevBuf plan_status;
    /* the one-launch plan's look-back states (zero between launches) */
    kgx::DevBuf plan_look;
    kgx::PinnedVec<uint32_t> h_plan_status;
    /* current plan */
    uint32_t n_seq = 0;
    uint64_t n_residues = 0;
    uint64_t max_tiles = 0;
    uint32_t tile_windows = 64u * kgx::PROBE_J_DEFAULT;
    uint64_t hit_slots = 0; /* slots per hit plane: cold plane at hits + hit_slots */
    const uint64_t *d_off = nullptr;
    bool have_hits = false; /* the tiled hits of the current plan are on the device */
    uint32_t hit_format = kgx::HIT_PLANES; /* of the current plan's hits (set by the probe) */
    bool have_best = false; /* best[] holds find_best_call of the current plan */
    bool defer_best = false; /* kgx_stage_score leaves best[] to the small path's collect */
    kgx::DevBuf best, best_ws, bc_calls, bc_start, bc_count; /* KGX_WANT_BEST / kgx_find_best_calls */
    kgx::PinnedVec<kgx_best_call> h_best;
    /* fq fragments (kgx_fq.hip) */
    kgx::DevBuf fq_bases, fq_roff, fq_nfrag, fq_fbase, fq_tmp, fq_res, fq_off, fq_read, fq_frame, fq_start,
        fq_anchor, fq_nres;
    kgx::DevBuf fq_look; /* fq_fused: tile counter | tile states */
    kgx::PinnedVec<uint64_t> h_fq_tot; /* fragments, residues of the last fq batch */
    kgx::FqPending fq_pend;             /* an enqueued fragment pass awaiting its finish */
    /* kgx_fq_proteins (kgx_fq.hip): the ids, per read its fragments and their
     * scan, per (read, frame) its tokens, per fragment anchor / length / token
     * / read / frame / record size, the record offsets and the text */
    kgx::DevBuf ft_ids, ft_idoff, ft_rcnt, ft_rbase, ft_tok6, ft_anchor, ft_len, ft_token, ft_read, ft_frame,
        ft_size, ft_off, ft_text;
    kgx::PinnedVec<uint64_t> h_ft_idoff;
    std::vector<hipEvent_t> ft_events; /* timing: start, uploaded, indexed, sized, written */
    float ft_ms[4] = {0, 0, 0, 0};     /* upload, scan and indices, sizes, write of the last call */
    /* kgx_fq_parse (kgx_fq_parse.hip): the uploaded text, per tile its state
     * map, entry state, event counts and their prefix, per lane its entry
     * state, and the call's sums */
    kgx::DevBuf fp_text, fp_map, fp_state, fp_lane, fp_cnt, fp_pre, fp_sum;
    kgx::PinnedVec<uint64_t> h_fp_sum;
    std::vector<hipEvent_t> fp_events; /* timing: upload start, parse start, parse end */
    kgx_fq_reads fp_last{};            /* what the last parse returned (zero once its buffers are written again) */
    /* kgx_fq_read_ids (kgx_fq_ids.hip): the chosen reads, per read its id's
     * offset within its tile, the tiles' sums and their prefix, the ids and
     * their offsets */
    kgx::DevBuf fi_index, fi_local, fi_cnt, fi_pre, fi_sum, fi_ids, fi_off;
    kgx::PinnedVec<uint32_t> h_fi_index;
    kgx::PinnedVec<uint64_t> h_fi_off;
    kgx::PinnedVec<char> h_fi_ids;
    uint64_t fq_ids_fetched = 0; /* ids kgx_fq_read_ids brought down */
    /* kgx_fa_parse (kgx_fa_parse.hip): the last FASTA text's residues, sequence
     * offsets, ids and id offsets; its scratch is the fp_* above */
    kgx::DevBuf fa_res, fa_soff, fa_ids, fa_idoff;
    /* kgx_gunzip / kgx_gunzip_device (kgx_gunzip.cpp) */
    kgx::DevBuf gz_in, gz_out, gz_members, gz_status, gz_stats;
    kgx::PinnedVec<kgx_gz_member> h_gz_members;
    kgx::PinnedVec<kgx_gz_status> h_gz_status;
    kgx::PinnedVec<kgx_inflate_stats> h_gz_stats;
    std::vector<hipEvent_t> gz_events; /* timing events: upload, kernel, download */
    /* kgx_fq_upload: reads whose H2D is enqueued, awaiting kgx_fq_fragments_uploaded */
    struct {
        bool active = false;
        uint32_t n_reads = 0;
        uint64_t n_bases = 0;
    } fq_up;
    kgx::PinnedVec<uint64_t> h_fq_roff; /* the uploaded reads' relative offsets (pinned: the copy is async) */
    /* kgx_fq_called_reads */
    kgx::DevBuf fqc_flag, fqc_reads, fqc_nsel, fqc_nfrag, fqc_ncall, fqc_fo, fqc_co, fqc_fc, fqc_len, fqc_coff,
        fqc_calls;
    kgx::PinnedVec<uint32_t> h_fqc_n, h_fqc_reads, h_fqc_fc, h_fqc_len;
    kgx::PinnedVec<uint64_t> h_fqc_tot, h_fqc_fo, h_fqc_coff;
    kgx::PinnedVec<kgx_call> h_fqc_calls;
    kgx::CtxOptions opt; /* the tuning options (kgx_ctx_set_option; kgx_options.h) */
    bool probe_defer = true; /* KGX_PROBE_DEFER at creation: the line probe's deferred form (kgx_probe.hip) */
    /* host results */
    std::vector<uint64_t> h_hoff, h_coff, h_ooff;
    kgx::PinnedVec<kgx_hit> h_hits;
    kgx::PinnedVec<kgx_call> h_calls;
    kgx::PinnedVec<kgx_otu> h_otus;
    kgx::PinnedVec<uint32_t> h_ocount;
    /* KGX_WANT_OTU: device tallies (otu_kernel) */
    kgx::DevBuf otu_ws, otus, otu_count, dense_ooff, dense_otus;
    bool have_otus = false;
    kgx::PinnedVec<uint32_t> h_hcount, h_ccount;
    kgx::PinnedVec<char> h_res;
    /* host-buffer batches in chunks (option "host_chunks"): the other context
     * the chunks alternate with */
    kgx_ctx *twin = nullptr;
    kgx::PinnedVec<uint64_t> h_off_stage, h_dense_hoff, h_dense_coff, h_dense_ooff, h_nwin;
    std::unique_ptr<kgx::HostPool> pool;       /* compact chunk D2H: the expansion threads (option "host_threads") */
    std::unique_ptr<kgx::HostPool> stage_pool; /* chunk staging threads (option "stage_threads") */
    kgx::PinnedVec<uint4> h_hits16;
    kgx::PinnedVec<uint64_t> h_mask;
    std::vector<uint64_t> h_wstart;     /* chunk-relative first window of each sequence */
    std::vector<hipEvent_t> chunk_done; /* per chunk: its records and mask are on the host */
    std::vector<hipEvent_t> chunk_counts; /* per chunk: its counts are on the host */
    std::vector<hipEvent_t> chunk_gathered; /* per chunk: its dense buffers are complete */
    hipStream_t copy_stream = nullptr; /* bulk chunk D2H, apart from the contexts' kernels */
    hipStream_t up_stream = nullptr; /* streamed schedule, option "host_upload_stream": the chunks' uploads */
    kgx::DevBuf up_res, up_off;
    kgx::DevBuf dense_mask, dense_best; /* a chunk's mask / best calls for its bulk copy */
    /* streamed schedule (option "host_stream"): records per window seen so far */
    double rate_hits = 0.35, rate_calls = 0.05, rate_otus = 0.05;
    uint64_t stream_fallbacks = 0; /* batches rerun exact after a region overflowed */
    bool one_pass_pinned = false; /* the enqueued one-pass batch reads caller-pinned residues */
    uint64_t pinned_batches = 0, nul_reruns = 0;
    uint64_t lean_scores = 0; /* score stages that launched score_lean_kernel */
    uint64_t fq_parses = 0;   /* texts framed on the device (kgx_fq_parse, kgx_fq_parse_device; n > 0) */
    uint32_t counts_enqueued = 0; /* want + 1 of an enqueued collect_counts_enqueue, else 0 */
    kgx::PinnedVec<uint32_t> h_nul;
    std::vector<hipEvent_t> chunk_h2d; /* per chunk: its staged residues are on the device */
    kgx::DevBuf dense_counts, cscan_ws;
    kgx::PinnedVec<uint32_t> h_counts;
    kgx::PinnedVec<uint32_t> h_hits12; /* 12-B records (3 words per hit, no key) */
    /* streamed, option "host_stage_all": every chunk's own staging region */
    kgx::PinnedVec<char> h_res_all;
    kgx::PinnedVec<uint64_t> h_off_all;
    /* small host batches (option "small_batch") */
    kgx::PinnedVec<uint4> h_small; /* offsets | window bases | tile owners | status | residues */
    kgx::PinnedVec<uint32_t> h_done; /* the fused small gather's completion token */
    kgx::DevBuf small_blocks_done;    /* its workgroup counter (zero between launches) */
    /* one-launch small batches (option "small_fused"; kgx_fused.hip): mapped
     * window bases, per-sequence result regions, counts and tokens */
    uint64_t fused_batches = 0, small_batches = 0; /* kgx_ctx_stat */
    kgx::PinnedVec<uint64_t> h_fwb;
    kgx::PinnedVec<kgx_hit> h_fhits;
    kgx::PinnedVec<kgx_call> h_fcalls;
    kgx::PinnedVec<uint32_t> h_fcounts, h_fdone;
    kgx::PinnedVec<uint64_t> h_fdbg; /* KGX_FUSED_DEBUG phase stamps */
    uint32_t small_token = 0;
    kgx::PinnedVec<kgx_call> h_calls_region;
    kgx::PinnedVec<kgx_otu> h_otus_region;
    /* compact results (kgx_process_batch_compact): the call leaves the hits as
     * records + mask; compact_segs say where each chunk's landed (element
     * offsets into h_hits12 / h_hits16 and h_mask, resolved to pointers once
     * the pinned arrays stop growing) */
    int compact_out = 0;
    struct CompactSeg {
        uint32_t s0, s1, words;
        uint64_t hit_begin, rec_at, mask_at;
    };
    std::vector<CompactSeg> compact_segs;
    std::vector<kgx_hit_chunk> compact_chunks;
    /* option "host_profile": per-chunk timing events and the last call's profile */
    std::vector<hipEvent_t> prof_ev; /* 4 per chunk: H2D start, H2D end, device end, gathered */
    std::vector<hipEvent_t> prof_done; /* per chunk: bulk copy done (timing events on the copy stream) */
    kgx_host_profile last_profile{};
    /* kgx_kmap_rollup */
    std::unique_ptr<kgx::RollupScratch> rollup;
};

namespace kgx {
static_assert(CtxOptions{}.probe_variant == PROBE_AUTO && CtxOptions{}.probe_j == PROBE_J_DEFAULT,
              "kgx_options.h spells these two defaults as numbers");
/* drops the image's line index, if any (the caller has set the device and
 * knows no kernel reads it) */
inline void drop_line_index(kgx_image *img)
{
    if (img->lines)
        (void)hipFree(img->lines.records);
    img->lines = LineIndex{};
}
/* what c's probes read: the image's line index unless option "line_index" is 0 */
inline bool ctx_lines(const kgx_ctx *c) { return c->img->lines && c->opt.line_index; }
inline ProbeTable ctx_probe_table(const kgx_ctx *c)
{
    ProbeTable t = ctx_lines(c) ? c->img->probe_table() : c->img->reference_table();
    t.filter = c->opt.probe_filter ? c->img->d_filter : nullptr;
    t.filter_log2_words = c->img->filter_log2_words;
    return t;
}
/* a host batch's result: the context's host arrays */
inline void fill_result(kgx_ctx *c, uint32_t n_seq, bool need_hits, bool want_best, uint64_t nwin, kgx_result *out)
{
    out->best = want_best ? c->h_best.data() : nullptr;
    out->n_seq = n_seq;
    out->hit_offsets = c->h_hoff.data();
    out->hits = need_hits ? c->h_hits.data() : nullptr;
    out->call_offsets = c->h_coff.data();
    out->calls = c->h_calls.data();
    out->otu_offsets = c->h_ooff.data();
    out->otus = c->h_otus.data();
    out->n_windows = nwin;
}

/* KGX_TIMING=1: phase wall times of the host-buffer path on stderr */
struct PhaseTimer {
    kgx_ctx *c;
    bool on;
    std::chrono::steady_clock::time_point t;
    explicit PhaseTimer(kgx_ctx *ctx) : c(ctx), on(std::getenv("KGX_TIMING") != nullptr), t(std::chrono::steady_clock::now()) {}
    void mark(const char *what)
    {
        if (!on)
            return;
        (void)hipStreamSynchronize(c->stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[kgx] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

/* one chunk of compact records -> kgx_hit for sequences [a, b) of it:
 * out[j - out_base] for CSR hit j (hoff: the batch's hit offsets);
 * kgx_hit.seq = s + seq_base; nt = streaming stores */
int expand_chunk(const kgx_hit_chunk &ch, const uint64_t *hoff, const char *residues, const uint64_t *seq_offsets,
                 uint32_t a, uint32_t b, kgx_hit *out, uint64_t out_base, uint32_t seq_base, bool nt);
/* kgx_compact_expand with a choice of streaming stores */
int compact_expand(const kgx_compact_result *r, const char *residues, const uint64_t *seq_offsets, uint32_t s_begin,
                   uint32_t s_end, uint32_t seq_base, kgx_hit *out, bool nt);
/* a corpus piece's n residues from the caller's src into c's pinned staging
 * and up to c->residues on c's stream, each sequence cut at its first NUL
 * (off: the piece's m + 1 absolute offsets); kgx_recall.hip */
int recall_stage_upload(kgx_ctx *c, const char *src, uint64_t n, const uint64_t *off, uint32_t m);
}  // namespace kgx

#endif
