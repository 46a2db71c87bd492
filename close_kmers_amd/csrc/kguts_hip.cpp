/*
 * kguts_hip.cpp -- the KmerGuts-compatible facade over the kgx C ABI.
 * Host-side rules restated from the reference: find_best_call
 * (kguts.cc:984-1199), text formatting (kguts.cc:939-973), OTU sorting
 * (kguts.h:185-219), index files (kguts.cc:544-575), FASTA framing
 * (fasta_parser.h:38-165, fasta_parser.cc:21-36).  The family data base and
 * the request handlers are in kguts_mapping.cpp, kguts_lookup.cpp and
 * kguts_fq.cpp.
 */
#include "kguts_impl.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cctype>
#include <cstring>
#include <iostream>

namespace kgx {

[[noreturn]] void throw_last(int rc, const std::string &what)
{
    throw Error(rc, what + ": " + kgx_strerror(rc) + " (" + kgx_last_error() + ")");
}

/* ---- stage clocks -------------------------------------------------------------- */

StageStats &stage_stats()
{
    static StageStats s;
    return s;
}

void StageStats::reset()
{
    for (auto *a : {&requests, &bytes_in, &bytes_out, &gpu_passes, &recv_ns, &parse_ns, &gpu_ns, &text_ns, &handle_ns,
                    &send_ns, &batched_pieces, &batched_passes})
        a->store(0);
    for (auto &a : text_cycles)
        a.store(0);
}

std::string StageStats::json() const
{
    char b[768];
    const double r = (double)std::max<uint64_t>(1, requests.load());
    std::snprintf(b, sizeof b,
                  "{\"requests\": %llu, \"bytes_in\": %llu, \"bytes_out\": %llu, \"gpu_passes\": %llu, "
                  "\"batched_pieces\": %llu, \"batched_passes\": %llu, "
                  "\"ms_per_request\": {\"recv\": %.4f, \"parse\": %.4f, \"gpu\": %.4f, \"text\": %.4f, \"handle\": %.4f, "
                  "\"send\": %.4f}, \"text_cycles\": [%llu, %llu, %llu, %llu, %llu]}\n",
                  (unsigned long long)requests.load(), (unsigned long long)bytes_in.load(),
                  (unsigned long long)bytes_out.load(), (unsigned long long)gpu_passes.load(),
                  (unsigned long long)batched_pieces.load(), (unsigned long long)batched_passes.load(),
                  recv_ns.load() / r * 1e-6,
                  parse_ns.load() / r * 1e-6, gpu_ns.load() / r * 1e-6, text_ns.load() / r * 1e-6,
                  handle_ns.load() / r * 1e-6,
                  send_ns.load() / r * 1e-6, (unsigned long long)text_cycles[0].load(),
                  (unsigned long long)text_cycles[1].load(), (unsigned long long)text_cycles[2].load(),
                  (unsigned long long)text_cycles[3].load(), (unsigned long long)text_cycles[4].load());
    return b;
}

StageClock::StageClock(std::atomic<uint64_t> &acc) : acc_(acc), t0_(now_ns()) {}
StageClock::~StageClock() { acc_ += now_ns() - t0_; }

/* ---- KmerOtuStats ----------------------------------------------------------- */

void KmerOtuStats::write(FILE *fh) const
{
    std::fprintf(fh, "OTU-COUNTS\t%s[%d]", contig_id.c_str(), contig_len);
    for (const auto &p : otus_by_count)
        std::fprintf(fh, "\t%d-%d", p.second, p.first);
    std::fprintf(fh, "\n");
}

void KmerOtuStats::finalize()
{
    otus_by_count.insert(otus_by_count.begin(), otu_map.begin(), otu_map.end());
    std::sort(otus_by_count.begin(), otus_by_count.end(),
              [](const std::pair<int, int> &l, const std::pair<int, int> &r) {
                  return r.second < l.second;
              });
}

/* ---- KmerImage ---------------------------------------------------------------- */

KmerImage::KmerImage(const std::string &data_dir, int device) : data_dir_(data_dir)
{
    int rc = kgx_image_open(data_dir.c_str(), device, &img_);
    if (rc)
        throw_last(rc, "KmerImage(" + data_dir + ")");
}

KmerImage::KmerImage(kgx_image *adopted) : img_(adopted)
{
    if (!img_)
        throw Error(KGX_EINVAL, "KmerImage: null image");
}

KmerImage::KmerImage(kgx_image *borrowed, bool owned) : img_(borrowed), owned_(owned)
{
    if (!img_)
        throw Error(KGX_EINVAL, "KmerImage: null image");
}

KmerImage::~KmerImage()
{
    if (owned_)
        kgx_image_close(img_);
}

/* ---- index files ----------------------------------------------------------- */

bool load_index_file(const std::string &path, std::vector<std::string> &out)
{
    FILE *f = std::fopen(path.c_str(), "r");
    if (!f)
        return false;
    out.clear();
    int idx;
    char line[1000];
    /* fscanf("%d\t") skips any whitespace after the number; fgets keeps the
     * newline, which the reference then overwrites (even if it is not one) */
    while (std::fscanf(f, "%d\t", &idx) == 1 && std::fgets(line, sizeof(line), f)) {
        if (idx != (int)out.size()) {
            std::fclose(f);
            return false;
        }
        size_t n = std::strlen(line);
        out.emplace_back(line, n ? n - 1 : 0);
    }
    std::fclose(f);
    return true;
}

/* ---- KmerGuts ------------------------------------------------------------------ */

KmerGuts::KmerGuts(const std::string &kmer_dir, std::shared_ptr<KmerImage> image) : image_(image)
{
    if (!image_)
        throw Error(KGX_EINVAL, "KmerGuts: null image");
    if (!load_index_file(kmer_dir + "/function.index", functions_))
        throw Error(KGX_EIO, "could not load " + kmer_dir + "/function.index");
    if (!load_index_file(kmer_dir + "/otu.index", otus_))
        throw Error(KGX_EIO, "could not load " + kmer_dir + "/otu.index");
    set_default_parameters();
    int rc = kgx_ctx_create(image_->handle(), &ctx_);
    if (rc)
        throw_last(rc, "kgx_ctx_create");
}

KmerGuts::~KmerGuts() { kgx_ctx_destroy(ctx_); }

bool KmerGuts::default_service()
{
    const char *e = std::getenv("KGX_SVC");
    return !(e && std::atoi(e) == 0);
}

void KmerGuts::set_default_parameters()
{
    kgx_params p;
    kgx_params_default(&p);
    order_constraint = p.order_constraint;
    min_hits = p.min_hits;
    min_weighted_hits = p.min_weighted_hits;
    max_gap = p.max_gap;
}

void KmerGuts::set_parameters(const std::map<std::string, std::string> &params)
{
    std::vector<const char *> names, values;
    for (const auto &kv : params) {
        names.push_back(kv.first.c_str());
        values.push_back(kv.second.c_str());
    }
    kgx_params p;
    int rc = kgx_params_parse(&p, names.data(), values.data(), names.size());
    if (rc)
        throw std::out_of_range(kgx_last_error()); /* std::stoi's own exception */
    order_constraint = p.order_constraint;
    min_hits = p.min_hits;
    min_weighted_hits = p.min_weighted_hits;
    max_gap = p.max_gap;
}

void KmerGuts::process_aa_batch(std::vector<SeqJob> &jobs)
{
    const uint32_t n = (uint32_t)jobs.size();
    std::vector<uint64_t> off(n + 1, 0);
    uint32_t want = 0;
    for (uint32_t i = 0; i < n; i++) {
        off[i + 1] = off[i] + jobs[i].seq.size();
        if (jobs[i].hit_cb)
            want |= KGX_WANT_HITS;
        if (jobs[i].calls)
            want |= KGX_WANT_CALLS;
        if (jobs[i].otu_stats)
            want |= KGX_WANT_OTU;
    }
    std::string buf;
    buf.reserve(off[n]);
    for (auto &j : jobs)
        buf += j.seq;
    kgx_params p{min_hits, max_gap, order_constraint, min_weighted_hits};
    /* compact hits: each sequence's hit_in_sequence_t are built as its
     * callbacks replay (no 32-B record per hit for the whole batch) */
    kgx_compact_result cr;
    int rc;
    {
        StageClock clk(stage_stats().gpu_ns);
        rc = kgx_process_batch_compact(ctx_, &p, buf.data(), off.data(), n, want, &cr);
    }
    stage_stats().gpu_passes++;
    if (rc)
        throw_last(rc, "kgx_process_batch_compact");
    const kgx_result &r = cr.r;
    std::vector<kgx_hit> seq_hits;
    for (uint32_t s = 0; s < n; s++) {
        SeqJob &j = jobs[s];
        if (j.hit_cb) {
            const uint64_t nh = r.hit_offsets[s + 1] - r.hit_offsets[s];
            seq_hits.resize(nh);
            if (nh && (rc = kgx_compact_expand(&cr, buf.data(), off.data(), s, s + 1, 0, seq_hits.data())))
                throw_last(rc, "kgx_compact_expand");
            for (uint64_t i = 0; i < nh; i++) {
                const kgx_hit &h = seq_hits[i];
                sig_kmer_t e;
                e.which_kmer = h.which_kmer;
                e.otu_index = h.otu_index;
                e.avg_from_end = h.avg_from_end;
                e.pad = 0;
                e.function_index = h.function_index;
                e.function_wt = h.function_wt;
                j.hit_cb(hit_in_sequence_t(e, h.pos));
            }
        }
        if (j.calls) {
            for (uint64_t i = r.call_offsets[s]; i < r.call_offsets[s + 1]; i++) {
                const kgx_call &c = r.calls[i];
                j.calls->push_back(KmerCall(c.start, c.end, c.count, c.function_index, c.weighted_hits));
            }
        }
        if (j.otu_stats) {
            for (uint64_t i = r.otu_offsets[s]; i < r.otu_offsets[s + 1]; i++)
                j.otu_stats->otu_map[r.otus[i].otu_index] += r.otus[i].count;
            j.otu_stats->finalize(); /* process_aa_seq, kguts.cc:906-907 */
        }
        if (j.on_done)
            j.on_done();
    }
}

/* ---- SeqCoalescer ------------------------------------------------------- */

SeqCoalescer::SeqCoalescer()
{
    if (const char *e = std::getenv("KGX_COALESCE_INFLIGHT"))
        max_inflight = std::max(1, std::atoi(e));
    if (const char *e = std::getenv("KGX_COALESCE_RESIDUES"))
        max_residues = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10));
    if (const char *e = std::getenv("KGX_COALESCE_SPIN_US"))
        spin_us = std::max(0, std::atoi(e));
}

void SeqCoalescer::submit(kgx_ctx *ctx, Req &r)
{
    using clock = std::chrono::steady_clock;
    {
        std::lock_guard<std::mutex> lk(mu_);
        queue_.push_back(&r);
        queued_.store(queue_.size(), std::memory_order_relaxed);
    }
    /* a waiter spins (a pass takes tens of us; a futex wake-up costs several)
     * and sleeps only after spin_us; it wakes for its own result or to lead */
    const auto spin_end = clock::now() + std::chrono::microseconds(spin_us);
    for (uint32_t spin = 0;; spin++) {
        if (r.done.load(std::memory_order_acquire))
            return;
        const bool can_lead = inflight_.load(std::memory_order_relaxed) < max_inflight &&
                              queued_.load(std::memory_order_relaxed) > 0;
        if (!can_lead && ((spin & 63u) != 0 || clock::now() < spin_end)) {
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            continue;
        }
        std::unique_lock<std::mutex> lk(mu_);
        if (r.done.load(std::memory_order_acquire))
            return;
        if (inflight_.load(std::memory_order_relaxed) < max_inflight && !queue_.empty()) {
            /* lead a pass: the queue's head and every queued call with the
             * same parameters, in arrival order, up to max_residues */
            std::vector<Req *> batch;
            uint64_t res = 0;
            const kgx_params p0 = queue_.front()->params;
            for (auto it = queue_.begin(); it != queue_.end();) {
                Req *q = *it;
                const bool same = q->params.min_hits == p0.min_hits && q->params.max_gap == p0.max_gap &&
                                  q->params.order_constraint == p0.order_constraint &&
                                  q->params.min_weighted_hits == p0.min_weighted_hits;
                if (same && (batch.empty() || res + q->seq->size() <= max_residues)) {
                    batch.push_back(q);
                    res += q->seq->size();
                    it = queue_.erase(it);
                } else {
                    ++it;
                }
            }
            queued_.store(queue_.size(), std::memory_order_relaxed);
            inflight_.fetch_add(1, std::memory_order_relaxed);
            lk.unlock();
            run_batch(ctx, batch);
            lk.lock();
            inflight_.fetch_sub(1, std::memory_order_relaxed);
            passes++;
            calls += batch.size();
            /* the callers served, and a sleeping queue head to lead the next
             * pass (spinning callers see the flags themselves) */
            for (Req *q : batch) {
                q->done.store(true, std::memory_order_release);
                if (q->sleeping)
                    q->cv.notify_one();
            }
            if (!queue_.empty() && queue_.front()->sleeping)
                queue_.front()->cv.notify_one();
            continue;
        }
        if (clock::now() < spin_end)
            continue; /* someone else leads: keep spinning */
        r.sleeping = true;
        r.cv.wait(lk, [&] {
            return r.done.load(std::memory_order_acquire) ||
                   (inflight_.load(std::memory_order_relaxed) < max_inflight && !queue_.empty());
        });
        r.sleeping = false;
    }
}

void SeqCoalescer::run_batch(kgx_ctx *ctx, std::vector<Req *> &batch)
{
    const uint32_t n = (uint32_t)batch.size();
    std::vector<uint64_t> off(n + 1, 0);
    uint32_t want = 0;
    for (uint32_t i = 0; i < n; i++) {
        off[i + 1] = off[i] + batch[i]->seq->size();
        want |= batch[i]->want;
    }
    std::string buf;
    buf.reserve(off[n]);
    for (Req *q : batch)
        buf += *q->seq;
    kgx_compact_result cr;
    /* per-sequence callers: the one-launch path where it applies */
    (void)kgx_ctx_set_option(ctx, "small_fused", 1);
    int rc = kgx_process_batch_compact(ctx, &batch[0]->params, buf.data(), off.data(), n, want, &cr);
    (void)kgx_ctx_set_option(ctx, "small_fused", 0);
    const kgx_result &r = cr.r;
    for (uint32_t i = 0; i < n && !rc; i++) {
        Req &q = *batch[i];
        if (q.want & KGX_WANT_HITS) {
            q.out.hits.resize(r.hit_offsets[i + 1] - r.hit_offsets[i]);
            if (!q.out.hits.empty())
                rc = kgx_compact_expand(&cr, buf.data(), off.data(), i, i + 1, 0, q.out.hits.data());
        }
        if (q.want & KGX_WANT_CALLS)
            q.out.calls.assign(r.calls + r.call_offsets[i], r.calls + r.call_offsets[i + 1]);
        if (q.want & KGX_WANT_OTU)
            q.out.otus.assign(r.otus + r.otu_offsets[i], r.otus + r.otu_offsets[i + 1]);
    }
    if (rc) {
        const std::string err = kgx_last_error();
        for (Req *q : batch) {
            q->rc = rc;
            q->err = err;
        }
    }
}

void KmerGuts::process_aa_seq(const std::string &id, const std::string &seq,
                              std::shared_ptr<std::vector<KmerCall>> calls,
                              std::function<void(hit_in_sequence_t)> hit_cb,
                              std::shared_ptr<KmerOtuStats> otu_stats)
{
    const uint32_t want = (hit_cb ? KGX_WANT_HITS : 0u) | (calls ? KGX_WANT_CALLS : 0u) | (otu_stats ? KGX_WANT_OTU : 0u);
    if (coalesce && service && want) {
        /* the image's resident call service: no launch on this call's path
         * (KGX_EBUSY: not a call it serves, or every slot taken -> below) */
        thread_local std::vector<kgx_hit> hbuf;
        thread_local std::vector<kgx_call> cbuf;
        thread_local std::vector<kgx_otu> obuf;
        const uint64_t W = seq.size() >= 9 ? seq.size() - 8 : 0;
        if (hbuf.size() < W)
            hbuf.resize(W);
        if (cbuf.size() < W)
            cbuf.resize(W);
        if (otu_stats && obuf.size() < W)
            obuf.resize(W);
        const kgx_params p{min_hits, max_gap, order_constraint, min_weighted_hits};
        uint64_t nh = 0, nc = 0, no = 0;
        const int rc = kgx_svc_call(image_->handle(), &p, seq.data(), seq.size(), want, hbuf.data(), hbuf.size(), &nh,
                                    cbuf.data(), cbuf.size(), &nc, obuf.data(), obuf.size(), &no);
        if (rc == KGX_OK) {
            /* replay on the calling thread, in position order (kguts.cc:814-815) */
            if (hit_cb)
                for (uint64_t i = 0; i < nh; i++) {
                    const kgx_hit &h = hbuf[i];
                    sig_kmer_t e;
                    e.which_kmer = h.which_kmer;
                    e.otu_index = h.otu_index;
                    e.avg_from_end = h.avg_from_end;
                    e.pad = 0;
                    e.function_index = h.function_index;
                    e.function_wt = h.function_wt;
                    hit_cb(hit_in_sequence_t(e, h.pos));
                }
            if (calls)
                for (uint64_t i = 0; i < nc; i++) {
                    const kgx_call &c = cbuf[i];
                    calls->push_back(KmerCall(c.start, c.end, c.count, c.function_index, c.weighted_hits));
                }
            if (otu_stats) {
                for (uint64_t i = 0; i < no; i++)
                    otu_stats->otu_map[obuf[i].otu_index] += obuf[i].count;
                otu_stats->finalize(); /* kguts.cc:906-907 */
            }
            return;
        }
        if (rc == KGX_EDEVICE) {
            /* no answer within 10 s leaves the service "broken" (every later
             * call KGX_EBUSY): replace it, so one stall does not turn the
             * service off for the rest of the process; this call takes the
             * batch path below */
            uint64_t broken = 0;
            if (kgx_svc_stat(image_->handle(), "broken", &broken) != KGX_OK || !broken)
                throw_last(rc, "kgx_svc_call");
            (void)kgx_svc_stop(image_->handle());
        } else if (rc != KGX_EBUSY) {
            throw_last(rc, "kgx_svc_call");
        }
    }
    if (coalesce) {
        SeqCoalescer::Req q;
        q.seq = &seq;
        q.params = kgx_params{min_hits, max_gap, order_constraint, min_weighted_hits};
        q.want = want;
        image_->coalescer().submit(ctx_, q);
        if (q.rc)
            throw Error(q.rc, "process_aa_seq: " + std::string(kgx_strerror(q.rc)) + " (" + q.err + ")");
        /* replay on the calling thread, in position order (kguts.cc:814-815) */
        if (hit_cb)
            for (const kgx_hit &h : q.out.hits) {
                sig_kmer_t e;
                e.which_kmer = h.which_kmer;
                e.otu_index = h.otu_index;
                e.avg_from_end = h.avg_from_end;
                e.pad = 0;
                e.function_index = h.function_index;
                e.function_wt = h.function_wt;
                hit_cb(hit_in_sequence_t(e, h.pos));
            }
        if (calls)
            for (const kgx_call &c : q.out.calls)
                calls->push_back(KmerCall(c.start, c.end, c.count, c.function_index, c.weighted_hits));
        if (otu_stats) {
            for (const kgx_otu &o : q.out.otus)
                otu_stats->otu_map[o.otu_index] += o.count;
            otu_stats->finalize(); /* kguts.cc:906-907 */
        }
        return;
    }
    /* one pass of one sequence: the one-launch path where it applies */
    struct Fused {
        kgx_ctx *c;
        explicit Fused(kgx_ctx *x) : c(x) { (void)kgx_ctx_set_option(c, "small_fused", 1); }
        ~Fused() { (void)kgx_ctx_set_option(c, "small_fused", 0); }
    } fused(ctx_);
    std::vector<SeqJob> jobs(1);
    jobs[0].id = id;
    jobs[0].seq = seq;
    jobs[0].calls = calls;
    jobs[0].hit_cb = hit_cb;
    jobs[0].otu_stats = otu_stats;
    process_aa_batch(jobs);
}

void KmerGuts::process_aa_seq_hits(const std::string &id, const std::string &seq,
                                   std::shared_ptr<std::vector<KmerCall>> calls,
                                   std::shared_ptr<std::vector<hit_in_sequence_t>> hits,
                                   std::shared_ptr<KmerOtuStats> otu_stats)
{
    /* kguts.cc:879-886 */
    auto cb = [hits](hit_in_sequence_t k) { hits->push_back(k); };
    process_aa_seq(id, seq, calls, cb, otu_stats);
}

const char *KmerGuts::function_at_index(int i) const
{
    if (i < 0 || i >= (int)functions_.size())
        return "INVALID_OFFSET";
    return functions_[i].c_str();
}

void KmerGuts::decoded_kmer(unsigned long long k, char *decoded)
{
    decoded[8] = 0;
    for (int i = 7; i >= 0; i--) {
        decoded[i] = kResidues[k % 20];
        k /= 20;
    }
}

unsigned long long KmerGuts::encoded_aa_kmer(const char *p)
{
    unsigned long long v = 0;
    for (int i = 0; i < 8; i++) {
        const char *hit = std::strchr(kResidues, p[i]);
        if (!p[i] || !hit)
            return 25600000000ULL + 1; /* MAX_ENCODED + 1 for any invalid residue */
        v = v * 20 + (unsigned long long)(hit - kResidues);
    }
    return v;
}

/* format_call / format_hit / format_otu_stats: iostream defaults (6
 * significant digits for floats), kguts.cc:939-973; append_* in kguts_impl.h */

extern "C" size_t kgx_format_g6(float v, char *out, size_t cap)
{
    char b[48];
    const size_t n = format_g6(b, sizeof b, v);
    if (out && cap) {
        const size_t k = std::min(n, cap - 1);
        std::memcpy(out, b, k);
        out[k] = 0;
    }
    return n;
}

void KmerGuts::append_call(std::string &out, const KmerCall &c) const
{
    out += "CALL\t";
    append_u64(out, c.start);
    out += '\t';
    append_u64(out, c.end);
    out += '\t';
    append_i64(out, c.count);
    out += '\t';
    append_u64(out, c.function_index);
    out += '\t';
    out += function_at_index((int)c.function_index);
    out += '\t';
    append_f32(out, c.weighted_hits);
    out += '\n';
}

void KmerGuts::append_hit(std::string &out, const hit_in_sequence_t &h) const
{
    char dc[9];
    decoded_kmer(h.hit.which_kmer, dc);
    out += "HIT\t";
    append_u64(out, h.offset);
    out += '\t';
    out += dc;
    out += '\t';
    append_u64(out, h.hit.avg_from_end);
    out += '\t';
    out += function_at_index(h.hit.function_index);
    out += '\t';
    append_f32(out, h.hit.function_wt);
    out += '\t';
    append_i64(out, h.hit.otu_index);
    out += '\n';
}

void KmerGuts::append_otu_stats(std::string &out, const std::string &id, size_t size,
                                const KmerOtuStats &s) const
{
    out += "OTU-COUNTS\t";
    out += id;
    out += '[';
    append_u64(out, size);
    out += ']';
    const size_t top = std::min<size_t>(s.otus_by_count.size(), 5);
    for (size_t i = 0; i < top; i++) {
        out += '\t';
        append_i64(out, s.otus_by_count[i].second);
        out += '-';
        append_i64(out, s.otus_by_count[i].first);
    }
    out += '\n';
}

std::string KmerGuts::format_call(const KmerCall &c)
{
    std::string o;
    append_call(o, c);
    return o;
}

std::string KmerGuts::format_hit(const hit_in_sequence_t &h)
{
    std::string o;
    append_hit(o, h);
    return o;
}

std::string KmerGuts::format_otu_stats(const std::string &id, size_t size, KmerOtuStats &s)
{
    std::string o;
    append_otu_stats(o, id, size, s);
    return o;
}

/* find_best_call, kguts.cc:1008-1199 -- a port of the SEED
 * km_process_hits_to_regions | km_pick_best_hit_in_peg pipeline. */
void KmerGuts::find_best_call(std::vector<KmerCall> &calls, int &function_index,
                              std::string &function, float &score, float &weighted_score,
                              float &score_offset)
{
    best_call(calls, [this](int i) { return function_at_index(i); }, function_index, function,
              score, weighted_score, score_offset);
}

void KmerGuts::find_best_call(const kgx_best_call &best, int &function_index, std::string &function,
                              float &score, float &weighted_score, float &score_offset)
{
    best_call(best, [this](int i) { return function_at_index(i); }, function_index, function, score,
              weighted_score, score_offset);
}

void best_call(const kgx_best_call &b, const std::function<const char *(int)> &name_of, int &function_index,
               std::string &function, float &score, float &weighted_score, float &score_offset)
{
    function_index = b.kind == 1 ? b.fi0 : -1;
    function.clear();
    score = b.score;
    weighted_score = b.weighted_score;
    if (b.kind != 0)
        score_offset = b.score_offset; /* kind 0: left as the caller had it */
    if (b.kind == 1) {
        function = name_of(b.fi0);
    } else if (b.kind == 2) { /* the lexically larger name first (kguts.cc:1176-1179) */
        std::string f1 = name_of(b.fi0), f2 = name_of(b.fi1);
        if (f2 > f1)
            std::swap(f1, f2);
        function = f1 + " ?? " + f2;
    }
}

void best_call(const std::vector<KmerCall> &calls, const std::function<const char *(int)> &name_of,
               int &function_index, std::string &function, float &score, float &weighted_score,
               float &score_offset)
{
    function_index = -1;
    function.clear();
    score = 0.0f;
    weighted_score = 0.0f;
    if (calls.empty())
        return; /* score_offset is left as the caller had it */

    /* adjacent calls of one function become one region */
    std::vector<KmerCall> regions;
    for (const KmerCall &c : calls) {
        if (!regions.empty() && regions.back().function_index == c.function_index) {
            KmerCall &r = regions.back();
            r.end = c.end;
            r.count += c.count;
            r.weighted_hits += c.weighted_hits;
        } else {
            regions.push_back(c);
        }
    }

    /* F1 | F2 | F1 with a weak interior (count < 5) and strong exterior
     * (counts summing to >= 10): drop F2 and join the F1 regions */
    std::vector<KmerCall> joined;
    size_t i = 0;
    while (i < regions.size()) {
        KmerCall cur = regions[i++];
        while (i + 1 < regions.size() && regions[i + 1].function_index == cur.function_index &&
               regions[i].count < 5 && cur.count + regions[i + 1].count >= 10) {
            cur.end = regions[i + 1].end;
            cur.count += regions[i + 1].count;
            cur.weighted_hits += regions[i + 1].weighted_hits;
            i += 2;
        }
        joined.push_back(cur);
    }

    /* per-function totals, ordered by function index (std::map) */
    typedef std::pair<int, std::pair<int, float>> total_t; /* fI -> (count, weighted) */
    std::map<int, std::pair<int, float>> totals;
    for (const KmerCall &c : joined) {
        auto ins = totals.emplace((int)c.function_index, std::make_pair(c.count, c.weighted_hits));
        if (!ins.second) {
            ins.first->second.first += c.count;
            ins.first->second.second += c.weighted_hits;
        }
    }
    std::vector<total_t> ranked(totals.begin(), totals.end());
    if (ranked.size() > 1)
        std::partial_sort(ranked.begin(), ranked.begin() + 2, ranked.end(),
                          [](const total_t &a, const total_t &b) {
                              return a.second.second > b.second.second;
                          });
    score_offset = ranked.size() == 1 ? (float)ranked[0].second.first
                                      : (float)(ranked[0].second.first - ranked[1].second.first);
    if (score_offset >= 5.0f) {
        function_index = ranked[0].first;
        function = name_of(function_index);
        score = (float)ranked[0].second.first;
        weighted_score = ranked[0].second.second;
        return;
    }
    /* ambiguous: optionally name the top two, lexically larger first */
    if (ranked.size() < 2)
        return;
    std::string a = name_of(ranked[0].first);
    std::string b = name_of(ranked[1].first);
    if (b > a)
        std::swap(a, b);
    if (ranked.size() == 2) {
        function = a + " ?? " + b;
        score = (float)ranked[0].second.first;
        return;
    }
    const float pair_offset = (float)(ranked[1].second.first - ranked[2].second.first);
    if (pair_offset > 5.0f) {
        function = a + " ?? " + b;
        score = (float)ranked[0].second.first;
        score_offset = pair_offset;
        weighted_score = ranked[0].second.second;
    }
}

/* ---- FastaParser --------------------------------------------------------------- */

FastaParser::FastaParser() { init_parse(); }

void FastaParser::init_parse()
{
    state_ = START;
    id_.clear();
    def_.clear();
    seq_.clear();
}

void FastaParser::emit()
{
    if (on_seq_)
        on_seq_(id_, seq_);
}

bool FastaParser::parse_char(char c)
{
    if (c == '\n')
        line_number_++;
    if (c == '\r')
        return true;
    std::string err;
    switch (state_) {
    case START:
        if (c == '>')
            state_ = ID;
        else
            err = "Missing >";
        break;
    case ID:
        if (std::isblank((unsigned char)c)) {
            def_.push_back(c);
            state_ = DEFLINE;
        } else if (c == '\n') {
            state_ = DATA;
        } else {
            id_.push_back(c);
        }
        break;
    case DEFLINE:
        if (c == '\n')
            state_ = DATA;
        else
            def_.push_back(c);
        break;
    case DATA:
        if (c == '\n')
            state_ = ID_OR_DATA;
        else if (std::isalpha((unsigned char)c) || c == '*')
            seq_.push_back(c);
        else
            err = std::string("Bad data character '") + c + "'";
        break;
    case ID_OR_DATA:
        if (c == '>') {
            emit();
            id_.clear();
            def_.clear();
            seq_.clear();
            state_ = ID;
        } else if (c == '\n') {
        } else if (std::isalpha((unsigned char)c)) {
            seq_.push_back(c);
            state_ = DATA;
        } else {
            err = std::string("Bad id or data character '") + c + "'";
        }
        break;
    }
    if (!err.empty()) {
        std::cerr << "Error found: " << err << " at line " << line_number_ << " id='" << id_ << "'"
                  << std::endl;
        if (on_error_)
            return on_error_(err, line_number_, id_);
    }
    return true;
}

void FastaParser::parse_complete()
{
    emit();
    id_.clear();
    def_.clear();
    seq_.clear();
}

void run_batch_on_device(KmerGuts &kg, const std::vector<std::string> &seqs)
{
    std::vector<uint64_t> off(seqs.size() + 1, 0);
    std::string buf;
    for (size_t i = 0; i < seqs.size(); i++) {
        buf += seqs[i];
        off[i + 1] = buf.size();
    }
    kgx_params p{kg.min_hits, kg.max_gap, kg.order_constraint, kg.min_weighted_hits};
    kgx_result r;
    int rc = kgx_process_batch(kg.ctx(), &p, buf.data(), off.data(), (uint32_t)seqs.size(), 0, &r);
    if (rc)
        throw_last(rc, "kgx_process_batch");
}

}  // namespace kgx

extern "C" int kgx_find_best_call(const kgx_call *calls, size_t n_calls, const char *const *names,
                                  int n_names, int32_t *function_index, char *function,
                                  size_t function_cap, float *score, float *weighted_score,
                                  float *score_offset, int *score_offset_set)
{
    if ((n_calls && !calls) || (n_names && !names) || !function_index || !score ||
        !weighted_score || !score_offset)
        return KGX_EINVAL;
    std::vector<kgx::KmerCall> v;
    v.reserve(n_calls);
    for (size_t i = 0; i < n_calls; i++)
        v.emplace_back(calls[i].start, calls[i].end, calls[i].count, calls[i].function_index,
                       calls[i].weighted_hits);
    auto name_of = [names, n_names](int i) -> const char * {
        return (i < 0 || i >= n_names) ? "INVALID_OFFSET" : names[i];
    };
    int fi;
    std::string fn;
    kgx::best_call(v, name_of, fi, fn, *score, *weighted_score, *score_offset);
    *function_index = fi;
    if (function && function_cap) {
        std::strncpy(function, fn.c_str(), function_cap - 1);
        function[function_cap - 1] = 0;
    }
    if (score_offset_set)
        *score_offset_set = n_calls > 0;
    return KGX_OK;
}
