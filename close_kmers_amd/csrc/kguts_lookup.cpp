/*
 * kguts_lookup.cpp -- the /lookup request of the facade: LookupBatcher
 * (concurrent requests' pieces in shared passes), the text helper threads
 * and LookupRequest (lookup_request.cc).
 */
#include "kguts_impl.h"
#include "kgx_score_map.h"

#include <algorithm>
#include <x86intrin.h>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <iostream>
#include <thread>

namespace kgx {

/* ---- LookupBatcher ------------------------------------------------------- */

struct LookupBatcher::Piece {
    uint32_t seq0 = 0, n = 0;
    uint64_t res0 = 0;
    Out *out = nullptr;
    int rc = KGX_OK;
    std::string err;
    bool done = false;
};

/* a staging area: pieces' residues and rebased offsets, contiguous, in
 * pinned host memory (the pass reads them by DMA, no staging copy) */
struct LookupBatcher::Area {
    char *res = nullptr;
    uint64_t *off = nullptr;
    uint64_t res_used = 0;
    uint32_t seq_used = 0, copying = 0;
    std::vector<Piece *> pieces;
    kgx_kmap *map = nullptr;
    int mode = 0;
    kgx_params p{};
    uint32_t want = 0;
    ~Area()
    {
        if (res)
            kgx_host_free(res);
        if (off)
            kgx_host_free(off);
    }
    bool fits(kgx_kmap *m, int md, const kgx_params &q, uint32_t w, uint64_t nres, uint32_t n, uint64_t max_res,
              uint32_t max_seq) const
    {
        if (pieces.empty())
            return true;
        return m == map && md == mode && w == want && q.min_hits == p.min_hits && q.max_gap == p.max_gap &&
               q.order_constraint == p.order_constraint && q.min_weighted_hits == p.min_weighted_hits &&
               res_used + nres <= max_res && seq_used + n <= max_seq;
    }
};

LookupBatcher::LookupBatcher(uint64_t max_residues, uint32_t max_seqs) : max_res_(max_residues), max_seq_(max_seqs)
{
    for (auto &a : area_)
        a.reset(new Area);
}

LookupBatcher::~LookupBatcher() = default;

void LookupBatcher::run_alone(KmerGuts &kg, kgx_kmap *map, int mode, const kgx_params &p, uint32_t want,
                              const char *res, const uint64_t *off, uint32_t n, Out &out)
{
    kgx_result r;
    int rc = kgx_process_batch(kg.ctx(), &p, res, off, n, want, &r);
    if (rc)
        throw_last(rc, "kgx_process_batch");
    kgx_rollup_result ru;
    if ((rc = kgx_kmap_rollup(map, kg.ctx(), mode, &ru)))
        throw_last(rc, "kgx_kmap_rollup");
    if (want & KGX_WANT_BEST)
        out.best.assign(r.best, r.best + n);
    out.roff.assign(ru.offsets, ru.offsets + n + 1);
    out.rows.assign(ru.rows, ru.rows + ru.offsets[n]);
}

void LookupBatcher::run(KmerGuts &kg, kgx_kmap *map, int mode, const kgx_params &p, uint32_t want,
                        const char *res, const uint64_t *off, uint32_t n, Out &out)
{
    const uint64_t nres = n ? off[n] - off[0] : 0;
    std::unique_lock<std::mutex> lk(mu_);
    /* alone (no other request inside), too large for an area, or a map the
     * worker's device cannot roll up in its own pass: the piece's own pass */
    const bool alone = active_ == 0 && !busy_ && area_[open_]->pieces.empty();
    if (alone || n == 0 || nres > max_res_ || n > max_seq_ ||
        kgx_kmap_device(map) != kgx_image_device(kg.image_->handle())) {
        active_++;
        lk.unlock();
        alone_++;
        try {
            run_alone(kg, map, mode, p, want, res, off, n, out);
        } catch (...) {
            lk.lock();
            active_--;
            throw;
        }
        lk.lock();
        active_--;
        return;
    }
    active_++;
    /* a place in the open area (wait while it holds other parameters or is full) */
    while (!area_[open_]->fits(map, mode, p, want, nres, n, max_res_, max_seq_))
        cv_.wait(lk);
    Area &A = *area_[open_];
    if (!A.res) { /* first use: both areas' pinned buffers */
        for (auto &a : area_) {
            void *r = nullptr, *o = nullptr;
            if (kgx_host_alloc(max_res_ + 64, &r) || kgx_host_alloc(((uint64_t)max_seq_ + 1) * 8, &o)) {
                if (r)
                    kgx_host_free(r);
                active_--;
                throw_last(KGX_ENOMEM, "lookup batcher: pinned staging");
            }
            a->res = static_cast<char *>(r);
            a->off = static_cast<uint64_t *>(o);
        }
    }
    Piece pc;
    pc.seq0 = A.seq_used;
    pc.res0 = A.res_used;
    pc.n = n;
    pc.out = &out;
    if (A.pieces.empty()) {
        A.map = map;
        A.mode = mode;
        A.p = p;
        A.want = want;
    }
    A.pieces.push_back(&pc);
    A.seq_used += n;
    A.res_used += nres;
    A.copying++;
    lk.unlock();
    /* the piece into place (each request copies its own, at once) */
    std::memcpy(A.res + pc.res0, res + off[0], nres);
    for (uint32_t i = 0; i < n; i++)
        A.off[pc.seq0 + i] = pc.res0 + (off[i] - off[0]);
    lk.lock();
    A.copying--;
    cv_.notify_all();
    Area *mine = &A;
    while (!pc.done) {
        /* no pass running and our area complete: lead it, the other area
         * (empty: its pass is over) opening for the next pieces */
        if (!busy_ && mine == area_[open_].get() && mine->copying == 0) {
            busy_ = true;
            open_ ^= 1;
            lk.unlock();
            lead(kg, *mine);
            lk.lock();
            for (Piece *q : mine->pieces)
                q->done = true;
            mine->pieces.clear();
            mine->seq_used = 0;
            mine->res_used = 0;
            busy_ = false;
            cv_.notify_all();
        } else {
            cv_.wait(lk);
        }
    }
    active_--;
    if (pc.rc)
        throw Error(pc.rc, "lookup batcher: " + pc.err);
}

void LookupBatcher::lead(KmerGuts &kg, Area &a)
{
    const uint32_t N = a.seq_used;
    a.off[N] = a.res_used;
    kgx_result r;
    kgx_rollup_result ru;
    const int rc = kgx_lookup(kg.ctx(), a.map, a.mode, &a.p, a.res, a.off, N, a.want, &r, &ru);
    passes_++;
    batched_ += a.pieces.size();
    stage_stats().batched_passes++;
    stage_stats().batched_pieces += a.pieces.size();
    const std::string err = rc ? kgx_last_error() : "";
    for (Piece *q : a.pieces) {
        q->rc = rc;
        if (rc) {
            q->err = err;
            continue;
        }
        Out &o = *q->out;
        if (a.want & KGX_WANT_BEST)
            o.best.assign(r.best + q->seq0, r.best + q->seq0 + q->n);
        const uint64_t r0 = ru.offsets[q->seq0], r1 = ru.offsets[q->seq0 + q->n];
        o.roff.resize((size_t)q->n + 1);
        for (uint32_t i = 0; i <= q->n; i++)
            o.roff[i] = ru.offsets[q->seq0 + i] - r0;
        o.rows.assign(ru.rows + r0, ru.rows + r1);
    }
}

/* ---- LookupRequest ------------------------------------------------------- */

static bool stoi_param(const std::map<std::string, std::string> &p, const char *k, int &out)
{
    /* std::stoi with only std::invalid_argument caught (lookup_request.cc:47-58) */
    auto it = p.find(k);
    if (it == p.end())
        return false;
    try {
        out = std::stoi(it->second);
        return true;
    } catch (const std::invalid_argument &) {
        return false;
    }
}

namespace {

/* Helper threads for a request's text stage: run(parts, fn) calls fn(0 ..
 * parts-1) once each, on the caller and on whichever helpers are idle (with
 * none idle the caller runs every part itself).  KGX_TEXT_HELPERS threads
 * (default 0: none; r8 at 16 clients on the box's 16-CPU share: 8.59e9
 * residues/s with none, 7.76e9 with 4, 7.34e9 with 8 -- the parts cost more
 * CPU than the share has spare), started on first use and never joined (a
 * process may exit with them waiting). */
class TextHelpers {
public:
    static TextHelpers &get()
    {
        static TextHelpers *h = new TextHelpers();
        return *h;
    }
    uint32_t size() const { return n_; }
    void run(uint32_t parts, const std::function<void(uint32_t)> &fn)
    {
        Job job{&fn, parts};
        const bool shared = n_ && parts > 1;
        if (shared) {
            std::lock_guard<std::mutex> g(mu_);
            jobs_.push_back(&job);
        }
        if (shared)
            cv_.notify_all();
        for (;;) {
            uint32_t p;
            {
                std::lock_guard<std::mutex> g(mu_);
                p = job.next < parts ? job.next++ : parts;
                if (job.next == parts && shared)
                    drop(&job);
            }
            if (p == parts)
                break;
            fn(p);
            std::lock_guard<std::mutex> g(mu_);
            job.done++;
        }
        std::unique_lock<std::mutex> lk(mu_);
        done_cv_.wait(lk, [&] { return job.done == parts; });
    }

private:
    struct Job {
        const std::function<void(uint32_t)> *fn;
        uint32_t parts;
        uint32_t next = 0, done = 0;
    };
    TextHelpers()
    {
        const char *e = std::getenv("KGX_TEXT_HELPERS");
        n_ = (uint32_t)std::max(0, std::min(64, e ? std::atoi(e) : 0));
        for (uint32_t i = 0; i < n_; i++)
            std::thread([this] { loop(); }).detach();
    }
    void drop(Job *j)
    {
        auto it = std::find(jobs_.begin(), jobs_.end(), j);
        if (it != jobs_.end())
            jobs_.erase(it);
    }
    void loop()
    {
        std::unique_lock<std::mutex> lk(mu_);
        for (;;) {
            cv_.wait(lk, [&] { return !jobs_.empty(); });
            Job *j = jobs_.front(); /* a queued job has parts left */
            const uint32_t p = j->next++;
            if (j->next == j->parts)
                jobs_.pop_front();
            lk.unlock();
            (*j->fn)(p);
            lk.lock();
            if (++j->done == j->parts)
                done_cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_, done_cv_;
    std::deque<Job *> jobs_;
    uint32_t n_ = 0;
};

}  // namespace

LookupRequest::LookupRequest(std::shared_ptr<KmerPegMapping> mapping, bool family_mode,
                             const std::map<std::string, std::string> &params)
    : mapping_(mapping), family_mode_(family_mode)
{
    int v;
    if (stoi_param(params, "kmer_hit_threhsold", v))
        kmer_hit_threshold_ = (unsigned int)v;
    if (stoi_param(params, "find_best_match", v))
        find_best_match_ = v != 0;
    if (stoi_param(params, "find_reps", v))
        find_reps_ = v != 0;
    if (stoi_param(params, "allow_ambiguous_functions", v))
        allow_ambiguous_functions_ = v != 0;
    auto tg_it = params.find("target_genus");
    const std::string tg = mapping_->lookup_genus(tg_it == params.end() ? std::string() : tg_it->second);
    try {
        if (!tg.empty())
            target_genus_id_ = std::stoul(tg);
    } catch (const std::invalid_argument &) {
    }
}

void LookupRequest::process_work(KmerGuts &kg, const std::vector<std::pair<std::string, std::string>> &work,
                                 std::ostream &os)
{
    std::string ids, res;
    std::vector<uint64_t> id_off{0}, off{0};
    for (const auto &w : work) {
        ids += w.first;
        id_off.push_back(ids.size());
        res += w.second;
        off.push_back(res.size());
    }
    process_flat(kg, res.data(), off.data(), ids.data(), id_off.data(), work.size(), os);
}

void LookupRequest::process_flat(KmerGuts &kg, const char *res, const uint64_t *off, const char *ids,
                                 const uint64_t *id_off, size_t n_work, std::ostream &os)
{
    /* pieces that keep the batch's hits on the device (one small-batch pass
     * each: at most 2M residues, 65,536 sequences) */
    const FlatWork fw{res, off, ids, id_off};
    size_t a = 0;
    while (a < n_work) {
        size_t b = a + 1;
        while (b < n_work && off[b + 1] - off[a] <= (uint64_t(1) << 21) && b - a < 65536)
            b++;
        process_piece(kg, fw, a, b, os);
        a = b;
    }
}

void LookupRequest::best_match_lines(KmerGuts &kg, const FlatWork &fw, size_t w0, uint32_t a, uint32_t b,
                                     const kgx_best_call *best, const uint64_t *roff, const kgx_rollup_row *rows,
                                     ScoreMap &smap, std::string &out) const
{
    typedef FamilyMapper::sequence_accumulated_score_t acc_t;
    /* the per-sequence strings live across the part's sequences: their
     * buffers are reused, not allocated per line */
    std::string id, fn, ambig, lf_fam, lf_fn, gf_fam;
    static const bool clocks = std::getenv("KGX_TEXT_CLOCKS") != nullptr;
    uint64_t cyc[5] = {0, 0, 0, 0, 0}, t_last = clocks ? __rdtsc() : 0;
    auto tick = [&](int k) {
        if (clocks) {
            const uint64_t t = __rdtsc();
            cyc[k] += t - t_last;
            t_last = t;
        }
    };
    /* a block's family lookups and name fetches first: independent of each
     * other, so their cache misses overlap instead of stalling one by one */
    constexpr uint32_t BLK = 16;
    std::vector<const KmerPegMapping::family_data_t *> fdv;
    uint64_t fd0 = 0;
    for (uint32_t s = a; s < b; s++) {
        if ((s - a) % BLK == 0) {
            const uint32_t e = std::min(b, s + BLK);
            fd0 = roff[s];
            fdv.resize(roff[e] - fd0);
            for (uint64_t j = fd0; j < roff[e]; j++) {
                auto it = mapping_->family_data_.find(rows[j].id);
                fdv[j - fd0] = it == mapping_->family_data_.end() ? nullptr : &it->second;
            }
            for (uint32_t q = s; q < e; q++)
                kg.prefetch_call_names(best[q]);
        }
        const size_t ia = fw.id_off[w0 + s], ib = fw.id_off[w0 + s + 1];
        id.assign(fw.ids + ia, ib - ia);
        /* smap as the reference's operator[] calls leave it: the ids in
         * first-touch order into the request's one map (cleared per sequence,
         * its bucket count kept), so its iteration order is the reference's */
        if (!smap.empty())
            smap.clear();
        fill_scores(smap, rows + roff[s], roff[s + 1] - roff[s]);
        tick(0);
        {
            int fi;
            float score, wscore, offs = 0.0f;
            ambig.clear();
            kg.find_best_call(best[s], fi, fn, score, wscore, offs);
            bool do_ambig = false;
            if (fn.empty()) {
                fn.assign("hypothetical protein");
            } else {
                const size_t where = fn.find(" ?? ");
                if (where != std::string::npos) {
                    if (allow_ambiguous_functions_) {
                        ambig = fn.substr(where + 4);
                        fn = fn.substr(0, where);
                        do_ambig = true;
                    } else {
                        fn = "hypothetical protein";
                    }
                }
            }
            tick(1);
            float lf_score = 0.0f, gf_score = 0.0f;
            lf_fam.clear();
            lf_fn.clear();
            gf_fam.clear();
            /* fresh maps per sequence, as the reference declares them
             * (lookup_request.cc:259): their iteration order -- the tie
             * order of the family pick below -- depends on it (an empty
             * map allocates nothing) */
            std::unordered_map<std::string, float> pgf_rollup, pgf_rollup_ambig;
            for (const auto &hit_ent : smap) {
                const acc_t &se = hit_ent.second;
                if (se.hit_total < kmer_hit_threshold_)
                    continue;
                /* the entry's family, looked up with the block (a search of
                 * the sequence's rows; past 32 rows the map again) */
                const KmerPegMapping::family_data_t *fdp = nullptr;
                if (roff[s + 1] - roff[s] <= 32) {
                    for (uint64_t j = roff[s]; j < roff[s + 1]; j++)
                        if (rows[j].id == hit_ent.first) {
                            fdp = fdv[j - fd0];
                            break;
                        }
                } else {
                    auto fent = mapping_->family_data_.find(hit_ent.first);
                    fdp = fent == mapping_->family_data_.end() ? nullptr : &fent->second;
                }
                if (!fdp)
                    continue;
                const KmerPegMapping::family_data_t &fd = *fdp;
                if (do_ambig) {
                    if (fd.function == fn)
                        pgf_rollup[fd.pgf] += se.weighted_total;
                    else if (fd.function == ambig)
                        pgf_rollup_ambig[fd.pgf] += se.weighted_total;
                    else
                        continue;
                } else {
                    if (fd.function == fn)
                        pgf_rollup[fd.pgf] += se.weighted_total;
                    else
                        continue;
                }
                if (se.weighted_total > lf_score && fd.genus_id == target_genus_id_) {
                    lf_score = se.weighted_total;
                    lf_fam = fd.plf;
                    lf_fn = fd.function;
                }
            }
            tick(2);
            auto *rollup = (do_ambig && lf_fn == ambig) ? &pgf_rollup_ambig : &pgf_rollup;
            for (const auto &pgf_ent : *rollup)
                if (pgf_ent.second > gf_score) {
                    gf_score = pgf_ent.second;
                    gf_fam = pgf_ent.first;
                }
            tick(3);
            /* the iostream line (lookup_request.cc), floats as operator<< prints them (%.6g) */
            out += id;
            out += '\t';
            out += gf_fam;
            out += '\t';
            append_f32(out, gf_score);
            out += '\t';
            out += lf_fam;
            out += '\t';
            append_f32(out, lf_score);
            out += '\t';
            out += do_ambig ? lf_fn : fn;
            out += '\t';
            append_f32(out, score);
            out += '\t';
            append_f32(out, wscore);
            out += '\n';
        }
        tick(4);
    }
    if (clocks)
        for (int k = 0; k < 5; k++)
            stage_stats().text_cycles[k] += cyc[k];
}

void LookupRequest::process_piece(KmerGuts &kg, const FlatWork &fw, size_t w0, size_t w1, std::ostream &os)
{
    const uint32_t n = (uint32_t)(w1 - w0);
    if (n == 0)
        return;
    const bool want_calls = find_best_match_ && family_mode_;
    kgx_params p{kg.min_hits, kg.max_gap, kg.order_constraint, kg.min_weighted_hits};
    kgx_result r;
    /* find_best_call runs on the device (KGX_WANT_BEST): only its decision
     * per sequence comes back, not the calls; the hits stay on the device,
     * where on_hit's rollups run (kgx_kmap_rollup) */
    const uint64_t g0 = now_ns(); /* gpu stage: the pass and the rollups */
    /* on_hit (lookup_request.cc:446-482) over kmer_to_family_id_ or kmer_to_id_ */
    kgx_kmap *map = family_mode_ ? mapping_->kmer_to_family_id() : mapping_->kmer_to_id();
    const int mode = family_mode_ ? KGX_ROLLUP_FAMILY : KGX_ROLLUP_PEG;
    const uint32_t want = want_calls ? KGX_WANT_BEST : 0u;
    kgx_rollup_result ru;
    /* the pass and the rollup enqueued together with one host wait
     * (kgx_lookup: the small-batch path with the rollup queued behind it)
     * when the map is on the worker's device; KGX_LOOKUP_ONE_WAIT=0: the
     * pass, then the rollup, a wait each (HTTP family /lookup at 16 clients
     * 9.05e9 vs 8.35e9 residues/s, r8 s20) */
    static const bool one_wait = [] {
        const char *e = std::getenv("KGX_LOOKUP_ONE_WAIT");
        return !e || std::atoi(e) != 0;
    }();
    int rc;
    const kgx_best_call *best = nullptr;
    const uint64_t *roff = nullptr;
    const kgx_rollup_row *rows = nullptr;
    LookupBatcher::Out out;
    if (batcher_) { /* a pass shared with concurrent requests' pieces */
        batcher_->run(kg, map, mode, p, want, fw.res, fw.off + w0, n, out);
        stage_stats().gpu_passes++;
        best = out.best.data();
        roff = out.roff.data();
        rows = out.rows.data();
    } else if (one_wait && kgx_kmap_device(map) == kgx_image_device(kg.image_->handle())) {
        rc = kgx_lookup(kg.ctx(), map, mode, &p, fw.res, fw.off + w0, n, want, &r, &ru);
        stage_stats().gpu_passes++;
        if (rc)
            throw_last(rc, "kgx_lookup");
        best = r.best;
        roff = ru.offsets;
        rows = ru.rows;
    } else {
        rc = kgx_process_batch(kg.ctx(), &p, fw.res, fw.off + w0, n, want, &r);
        stage_stats().gpu_passes++;
        if (rc)
            throw_last(rc, "kgx_process_batch");
        rc = kgx_kmap_rollup(map, kg.ctx(), mode, &ru);
        if (rc)
            throw_last(rc, "kgx_kmap_rollup");
        best = r.best;
        roff = ru.offsets;
        rows = ru.rows;
    }
    stage_stats().gpu_ns += now_ns() - g0;
    StageClock text_clock(stage_stats().text_ns); /* the scoring and the output lines, to the end */
    typedef FamilyMapper::sequence_accumulated_score_t acc_t;
    if (want_calls) {
        /* the lines in parts on the text helpers (KGX_TEXT_HELPERS): part k
         * starts from a map grown as the request's seq_score_ would be at
         * its first sequence, so every map iterates as the reference's one
         * does; the parts' text is written in order */
        TextHelpers &th = TextHelpers::get();
        const uint32_t P = std::max<uint32_t>(1u, std::min<uint32_t>(th.size() + 1, n / 768));
        std::vector<uint32_t> cut(P + 1);
        for (uint32_t k = 0; k <= P; k++)
            cut[k] = (uint32_t)((uint64_t)n * k / P);
        std::vector<size_t> most(P);
        size_t m = seq_score_most_;
        for (uint32_t k = 0, q = 0; k < P; k++) {
            most[k] = m;
            for (; q < cut[k + 1]; q++)
                m = std::max<size_t>(m, (size_t)(roff[q + 1] - roff[q]));
        }
        std::vector<std::string> outs(P);
        th.run(P, [&](uint32_t k) {
            if (k == 0) {
                best_match_lines(kg, fw, w0, cut[0], cut[1], best, roff, rows, seq_score_, outs[0]);
                return;
            }
            ScoreMap score;
            grow_to(score, most[k]);
            best_match_lines(kg, fw, w0, cut[k], cut[k + 1], best, roff, rows, score, outs[k]);
        });
        for (const std::string &o : outs)
            os.write(o.data(), (std::streamsize)o.size());
        if (P > 1) {
            seq_score_.clear();
            grow_to(seq_score_, m);
        }
        seq_score_most_ = m;
        return;
    }
    std::string id;
    for (uint32_t s = 0; s < n; s++) {
        const size_t ia = fw.id_off[w0 + s], ib = fw.id_off[w0 + s + 1];
        id.assign(fw.ids + ia, ib - ia);
        /* seq_score_ as the reference's operator[] calls leave it: the ids in
         * first-touch order into the request's one map (cleared per sequence,
         * its bucket count kept), so its iteration order is the reference's */
        if (!seq_score_.empty())
            seq_score_.clear();
        fill_scores(seq_score_, rows + roff[s], roff[s + 1] - roff[s]);
        {
            typedef std::pair<KmerPegMapping::encoded_id_t, acc_t> data_t;
            std::vector<data_t> vec(seq_score_.begin(), seq_score_.end());
            std::sort(vec.begin(), vec.end(), [](const data_t &l, const data_t &rr) {
                return l.second.weighted_total > rr.second.weighted_total;
            });
            os << id << "\n";
            for (auto &it : vec) {
                const acc_t &se = it.second;
                if (se.hit_total < kmer_hit_threshold_)
                    break;
                if (family_mode_) {
                    const KmerPegMapping::family_data_t fd = mapping_->family_at(it.first);
                    const float scaled = (float)se.hit_count / (float)fd.total_size;
                    os << se.hit_count << "\t" << se.hit_total << "\t" << se.weighted_total << "\t" << fd.pgf << "\t"
                       << fd.plf << "\t" << fd.total_size << "\t" << fd.count << "\t" << scaled << "\t"
                       << fd.function << "\n";
                    if (find_reps_)
                        os << "///\n"; /* no family reps DB loaded */
                } else {
                    os << mapping_->decode_id(it.first) << "\t" << se.hit_count;
                    auto fh = mapping_->peg_to_family_.find(it.first);
                    if (fh != mapping_->peg_to_family_.end()) {
                        const KmerPegMapping::family_data_t fd = mapping_->family_at(fh->second);
                        os << "\t" << fd.pgf << "\t" << fd.plf << "\t" << fd.function << "\n";
                    } else {
                        os << "\n";
                    }
                }
            }
            os << "//\n";
        }
    }
}

}  // namespace kgx
