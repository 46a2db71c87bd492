/*
 * kguts_fq.cpp -- the fq request handler of the facade: FqRequest
 * (FqProcessRequest, fq_process_request.cc:230-365) and its C ABI
 * (include/kgx.h kgx_fq_*).  A block of FASTQ, text or gzip (GzipBodyReader,
 * kgx_gzip.h), is cut into parts that are parsed ahead on worker threads
 * (FqParts); the parts rotate over three contexts (process_text), and each
 * part's reads get their frame chosen on the host (finish_block,
 * choose_frame).  With the context's option "fq_body_device" at 1 when a
 * request starts, the parts are framed on the device instead (DeviceBody,
 * DESIGN.md §8.14): plain byte cuts, the text behind a part's last complete
 * record carried in front of the next, a gzip body's blocked members inflated
 * on the device into the text the parser reads, and only the ids of the reads
 * that are printed brought down.
 */
#include "kguts_impl.h"
#include "kgx_fq_body.h"  /* FqBodyParts: the parts of a block the device frames */
#include "kgx_fq_parse.h" /* fq_parse: FastqParser::parse_char as the fq handler drives it */
#include "kgx_gzip.h"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <numeric>
#include <sstream>
#include <thread>

namespace kgx {

namespace {

/* a place to cut a FASTQ block for a parallel parse: a line that starts
 * with '@' and whose next-but-one line starts with '+' (a record start in
 * any well-formed file), searched from p for up to 1 MiB; null if none */
const char *fq_cut_after(const char *p, const char *end)
{
    const char *limit = std::min(end, p + (1 << 20));
    while (p < limit) {
        const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(limit - p)));
        if (!nl || nl + 1 >= end)
            return nullptr;
        const char *l0 = nl + 1;
        if (*l0 == '@') {
            const char *n1 = static_cast<const char *>(std::memchr(l0, '\n', (size_t)(end - l0)));
            const char *n2 = n1 ? static_cast<const char *>(std::memchr(n1 + 1, '\n', (size_t)(end - n1 - 1))) : nullptr;
            if (!n2)
                return nullptr;
            if (n2 + 1 < end && n2[1] == '+')
                return l0;
        }
        p = l0;
    }
    return nullptr;
}

/* KGX_FQ_PART_KB: the part size, for tests of the parts (default 32 MB, at least 4 KB) */
size_t fq_part_bytes()
{
    const char *e = std::getenv("KGX_FQ_PART_KB");
    return e ? std::max<size_t>(4, std::strtoull(e, nullptr, 10)) << 10 : size_t(32) << 20;
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

/* ---- FqPart: one part of a block, parsed ---------------------------------- */

/* its reads' bases in pinned host memory (kgx_host_alloc; the device copies
 * them from there), offsets, ids, and the parser state at its end */
struct FqRequest::FqPart {
    int state = 0;
    std::string id;
    char *bases = nullptr;
    size_t cap = 0, len = 0;
    std::vector<uint64_t> roff{0}, id_off{0};
    std::string id_chars;
    FqPart() = default;
    FqPart(const FqPart &) = delete;
    FqPart &operator=(const FqPart &) = delete;
    ~FqPart()
    {
        if (bases)
            kgx_host_free(bases);
    }
    /* empty, from a parser state, room for `need` bases */
    void begin(size_t need, int st, const std::string &carried_id, const char *carried_bases, size_t n_carried)
    {
        if (need > cap) {
            if (bases)
                kgx_host_free(bases);
            bases = nullptr;
            cap = 0;
            void *q = nullptr;
            const size_t want = need + need / 8 + 4096;
            int rc = kgx_host_alloc(want, &q);
            if (rc)
                throw_last(rc, "kgx_host_alloc");
            bases = static_cast<char *>(q);
            cap = want;
        }
        state = st;
        id = carried_id;
        if (n_carried)
            std::memcpy(bases, carried_bases, n_carried);
        len = n_carried;
        roff.assign(1, 0);
        id_off.assign(1, 0);
        id_chars.clear();
    }
    void parse(const char *a, const char *b) { fq_parse(a, b, state, id, bases, len, roff, id_chars, id_off); }
    /* parse_complete(): the record in progress is emitted as it stands */
    void complete()
    {
        id_chars += id;
        id_off.push_back(id_chars.size());
        roff.push_back(len);
        id.clear();
    }
    /* the parse stands at a record start with nothing pending */
    bool at_record_start() const { return state == FQ_START && id.empty() && len == roff.back(); }
    FqBlock view() const
    {
        FqBlock v;
        v.res = bases;
        v.roff = roff.data();
        v.ids = id_chars.data();
        v.id_off = id_off.data();
        v.n = id_off.size() - 1;
        return v;
    }
};

/* ---- FqParts: a block's parts, in order ------------------------------------ */

/* The block is cut into parts of about KGX_FQ_PART_KB at record starts
 * (fq_cut_after).  Worker threads parse the parts ahead, in order, into
 * pinned buffers (a ring of a few per worker); the request's thread takes
 * them in order.  Part 0 continues the carried parser state; the others
 * start speculatively in the start state, and a part is used only if the
 * exact sequential parse reaches its first byte in that state with nothing
 * pending (the previous record emitted).  Otherwise the rest of the block is
 * parsed again on the request's thread from the true state, as the block's
 * last part.  So the reads are the sequential parse's.  A block of one part
 * is parsed on the request's thread and starts no thread.  The last part
 * hands the block's end state back to the request. */
class FqRequest::FqParts {
public:
    explicit FqParts(FqRequest &rq) : rq_(rq) {}
    ~FqParts() { close(); }
    /* a block to cut; its workers start */
    void open(const char *text, size_t n, bool finished);
    /* the workers stopped and joined (the parts handed out stay valid) */
    void close();
    size_t planned() const { return K_; } /* the cuts' parts: a re-parse of the rest ends the block sooner */
    /* part j, given part j - 1 (null for part 0); *last: the block ends with it */
    FqPart &get(size_t j, const FqPart *prev, bool *last);
    /* part j is done with: its buffer may take a later part */
    void release(size_t j);
    double wait_ms = 0.0; /* get() waiting for the workers, this block */

private:
    void work();
    void parse_cut(FqPart &pt, size_t k);
    void finish_part(FqPart &pt);
    FqRequest &rq_;
    /* kept across blocks, so the pinned buffers are allocated once: the ring,
     * and the exact re-parse after a rejected speculative cut */
    std::vector<std::unique_ptr<FqPart>> ring_;
    std::unique_ptr<FqPart> tail_;
    /* the open block */
    const char *end_ = nullptr;
    bool finished_ = false;
    std::vector<const char *> cuts_;
    size_t K_ = 0, R_ = 0; /* parts; ring slots in use */
    std::mutex mu_;
    std::condition_variable cv_;
    size_t next_ = 0, consumed_ = 0, tail_at_ = SIZE_MAX;
    bool abort_ = false;
    std::vector<size_t> ready_; /* ring slot -> the part it holds, parsed */
    std::string err_;
    std::vector<std::thread> pool_;
};

void FqRequest::FqParts::open(const char *text, size_t n, bool finished)
{
    const size_t kPartBytes = fq_part_bytes();
    end_ = text + n;
    finished_ = finished;
    cuts_.assign(1, text);
    const size_t want_parts = n / kPartBytes;
    /* the first part is an eighth of the others: nothing overlaps its parse
     * (r5k: 4.4-5.9 ms of a 66-ms block waiting for a 32-MB first part) */
    if (want_parts > 1)
        if (const char *c = fq_cut_after(text + kPartBytes / 8, end_))
            cuts_.push_back(c);
    for (size_t i = 1; i < want_parts; i++) {
        const char *c = fq_cut_after(text + n * i / want_parts, end_);
        if (c && c > cuts_.back())
            cuts_.push_back(c);
    }
    cuts_.push_back(end_);
    K_ = cuts_.size() - 1;
    wait_ms = 0.0;
    tail_at_ = SIZE_MAX;
    const size_t W =
        K_ == 1 ? 0 : std::min<size_t>(K_, std::max<size_t>(1, std::min<size_t>(15, std::thread::hardware_concurrency() - 1)));
    R_ = std::min(K_, 2 * W + 2); /* parts in flight */
    while (ring_.size() < R_)
        ring_.emplace_back(new FqPart);
    if (W == 0)
        return;
    next_ = consumed_ = 0;
    abort_ = false;
    ready_.assign(R_, SIZE_MAX);
    err_.clear();
    for (size_t w = 0; w < W; w++)
        pool_.emplace_back([this] { work(); });
}

/* part k as its cut says: part 0 from the request's carried state (which
 * only the block's last part changes), the others from the start state */
void FqRequest::FqParts::parse_cut(FqPart &pt, size_t k)
{
    const size_t span = (size_t)(cuts_[k + 1] - cuts_[k]);
    if (k == 0)
        pt.begin(rq_.seq_.size() + span, rq_.state_, rq_.id_, rq_.seq_.data(), rq_.seq_.size());
    else
        pt.begin(span, FQ_START, std::string(), nullptr, 0);
    pt.parse(cuts_[k], cuts_[k + 1]);
}

void FqRequest::FqParts::work()
{
    for (;;) {
        size_t k;
        {
            std::unique_lock<std::mutex> lk(mu_);
            if (abort_ || next_ >= K_)
                return;
            k = next_++;
            cv_.wait(lk, [&] { return abort_ || k < consumed_ + R_; });
            if (abort_)
                return;
        }
        FqPart &pt = *ring_[k % R_];
        try {
            parse_cut(pt, k);
        } catch (const std::exception &e) {
            std::lock_guard<std::mutex> lk(mu_);
            err_ = e.what();
            abort_ = true;
            cv_.notify_all();
            return;
        }
        std::lock_guard<std::mutex> lk(mu_);
        ready_[k % R_] = k;
        cv_.notify_all();
    }
}

void FqRequest::FqParts::close()
{
    if (pool_.empty())
        return;
    {
        std::lock_guard<std::mutex> lk(mu_);
        abort_ = true;
    }
    cv_.notify_all();
    for (auto &th : pool_)
        th.join();
    pool_.clear();
}

/* the final part: the block's end state goes back to the request */
void FqRequest::FqParts::finish_part(FqPart &pt)
{
    if (finished_) { /* parse_complete() emits the last record */
        pt.complete();
        rq_.state_ = FQ_START;
        rq_.id_.clear();
        rq_.seq_.clear();
    } else { /* the cut record's residues wait for the next block */
        rq_.state_ = pt.state;
        rq_.id_ = pt.id;
        rq_.seq_.assign(pt.bases + pt.roff.back(), pt.len - pt.roff.back());
    }
}

FqRequest::FqPart &FqRequest::FqParts::get(size_t j, const FqPart *prev, bool *last)
{
    *last = true;
    if (K_ == 1) { /* the whole block, here */
        FqPart &pt = *ring_[0];
        parse_cut(pt, 0);
        finish_part(pt);
        return pt;
    }
    if (prev && !prev->at_record_start()) {
        /* the cut was no record start: the rest of the block again, from prev's end state */
        close();
        if (!tail_)
            tail_.reset(new FqPart);
        const size_t pending = prev->len - prev->roff.back();
        tail_->begin((size_t)(end_ - cuts_[j]) + pending, prev->state, prev->id, prev->bases + prev->roff.back(), pending);
        tail_->parse(cuts_[j], end_);
        finish_part(*tail_);
        tail_at_ = j;
        return *tail_;
    }
    const auto w0 = std::chrono::steady_clock::now();
    {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return ready_[j % R_] == j || !err_.empty(); });
        if (!err_.empty())
            throw std::runtime_error(err_);
    }
    wait_ms += ms_since(w0);
    FqPart &pt = *ring_[j % R_];
    *last = j + 1 == K_;
    if (*last)
        finish_part(pt);
    return pt;
}

void FqRequest::FqParts::release(size_t j)
{
    if (K_ == 1 || j == tail_at_)
        return;
    std::lock_guard<std::mutex> lk(mu_);
    ready_[j % R_] = SIZE_MAX;
    consumed_ = j + 1;
    cv_.notify_all();
}

/* ---- option "fq_body_device": parts framed on the device -------------------- */

/* What the device-framed path keeps between parts and blocks.  The carried
 * text -- parts.have() bytes behind the last complete record -- is in `part`
 * (a text body) or in d_text[cur] at tail_off (a gzip body, whose text never
 * comes down but for the request's last incomplete record). */
struct FqRequest::DeviceBody {
    FqBodyParts parts;
    int device = 0;
    char *part = nullptr; /* a part's text on the host, pinned (kgx_host_alloc): carried text, then new bytes */
    size_t part_cap = 0;
    void *d_gz = nullptr; /* a gzip block's compressed bytes */
    size_t d_gz_cap = 0;
    char *d_text[2] = {nullptr, nullptr}; /* a gzip body's parts alternate: the carry is copied from one to the other */
    size_t d_text_cap[2] = {0, 0};
    int cur = 0;
    uint64_t tail_off = 0;
    bool tail_on_device = false;
    FqPart host_part; /* a part the host parser makes: a request's end, a record too long for the device */

    DeviceBody() = default;
    DeviceBody(const DeviceBody &) = delete;
    DeviceBody &operator=(const DeviceBody &) = delete;
    ~DeviceBody()
    {
        if (part)
            kgx_host_free(part);
        for (void *p : {d_gz, (void *)d_text[0], (void *)d_text[1]})
            if (p)
                kgx_device_free(p);
    }
    void forget()
    {
        parts.forget();
        tail_on_device = false;
        tail_off = 0;
    }
    /* `part` holds need bytes; its first `keep` stay */
    void host_room(size_t need, size_t keep)
    {
        if (need <= part_cap)
            return;
        void *q = nullptr;
        const size_t want = need + need / 4 + 4096;
        if (int rc = kgx_host_alloc(want, &q))
            throw_last(rc, "kgx_host_alloc");
        if (keep)
            std::memcpy(q, part, keep);
        if (part)
            kgx_host_free(part);
        part = static_cast<char *>(q);
        part_cap = want;
    }
    /* a device buffer of at least need bytes; what it held is not kept */
    void device_room(void **p, size_t *cap, size_t need)
    {
        if (need <= *cap)
            return;
        if (*p)
            kgx_device_free(*p);
        *p = nullptr;
        *cap = 0;
        const size_t want = need + need / 4 + 4096;
        if (int rc = kgx_device_alloc(device, want, p))
            throw_last(rc, "kgx_device_alloc");
        *cap = want;
    }
    /* the carried text into `part` (a request's end; a plain member's text behind blocked ones) */
    void tail_to_host()
    {
        if (!tail_on_device)
            return;
        const uint64_t have = parts.have();
        if (have) {
            host_room((size_t)have, 0);
            if (int rc = kgx_memcpy_d2h(part, d_text[cur] + tail_off, have))
                throw_last(rc, "kgx_memcpy_d2h");
        }
        tail_on_device = false;
        tail_off = 0;
    }
    /* part[0, total) through the host parser from the start state: its
     * complete records, and with `finished` the record in progress
     * (parse_complete), as host_part; what follows the last complete record
     * is carried otherwise.  Null when that makes no read. */
    FqPart *host_rest(size_t total, bool finished)
    {
        host_part.begin(total, FQ_START, std::string(), nullptr, 0);
        size_t consumed = 0;
        const char *p = part, *end = part + total;
        while (p < end) { /* line by line: where the last complete record ends */
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            const char *q = nl ? nl + 1 : end;
            const size_t before = host_part.roff.size();
            host_part.parse(p, q);
            if (host_part.roff.size() != before)
                consumed = (size_t)(q - part);
            p = q;
        }
        if (finished) {
            host_part.complete();
            forget();
        } else {
            if (consumed && total > consumed)
                std::memmove(part, part + consumed, total - consumed);
            parts.carried(total - consumed);
            tail_on_device = false;
        }
        return host_part.roff.size() > 1 ? &host_part : nullptr;
    }
};

/* a part of a block as the rotation takes it: reads the device framed, or a
 * part the host parser made */
struct FqRequest::DevicePart {
    kgx_fq_reads reads{};
    FqPart *host = nullptr;
};

FqRequest::DeviceBody &FqRequest::device_body()
{
    if (!dev_) {
        dev_.reset(new DeviceBody);
        dev_->device = kgx_image_device(kg_.image_->handle());
        dev_->parts.reset(fq_part_bytes(), KGX_FQ_PARSE_MAX);
    }
    return *dev_;
}

/* ---- FqRequest -------------------------------------------------------------- */

FqRequest::FqRequest(KmerGuts &kg, std::shared_ptr<KmerPegMapping> mapping)
    : kg_(kg), mapping_(mapping), parts_(new FqParts(*this)), body_(new GzipBodyReader)
{
}

FqRequest::~FqRequest()
{
    for (kgx_ctx *c : twin_)
        if (c)
            kgx_ctx_destroy(c);
}

void FqRequest::process(const std::string &block, bool finished, std::ostream &os)
{
    process(block.data(), block.size(), finished, os);
}

void FqRequest::process(const char *block, size_t n, bool finished, std::ostream &os)
{
    const bool fresh = state_ == FQ_START && id_.empty() && seq_.empty() && !(dev_ && dev_->parts.have());
    if (fresh && body_->body() == GZ_BODY_UNKNOWN) { /* a request starts: its choice holds to its end */
        int64_t v = 0;
        if (int rc = kgx_ctx_get_option(kg_.ctx(), "fq_body_device", &v))
            throw_last(rc, "kgx_ctx_get_option");
        body_device_ = v != 0;
    }
    const char *text = nullptr;
    size_t len = 0;
    bool listed = false;
    if (int rc = body_device_ ? body_->feed_listed(kg_.ctx(), block, n, finished, fresh, &text, &len, &listed)
                              : body_->feed(kg_.ctx(), block, n, finished, fresh, &text, &len)) {
        /* bad gzip data: the parser forgets the request too */
        state_ = FQ_START;
        id_.clear();
        seq_.clear();
        if (dev_)
            dev_->forget();
        throw_last(rc, "kgx_gunzip");
    }
    if (!body_device_) {
        if (!text) /* held: too short to tell text from gzip yet */
            return;
        if (body_->gzip() && !len && !finished) /* no complete member yet */
            return;
        if (body_->gzip())
            stats_.host_members += body_->last_members();
        process_text(text, len, finished, os);
        return;
    }
    try {
        if (listed) { /* blocked members: inflated on the device, part by part */
            process_members_device(finished, os);
        } else if (text && !(body_->gzip() && !len && !finished)) {
            if (body_->gzip())
                stats_.host_members += body_->last_members();
            process_text_device(text, len, finished, os);
        }
    } catch (...) { /* the request is forgotten: the next block starts one */
        body_->reset();
        if (dev_)
            dev_->forget();
        throw;
    }
}

/* ---- option "fq_body_device": the parts' rotation and sources ------------- */

namespace {

/* memcpy by a few threads for a part's 32 MB */
void copy_bytes(char *dst, const char *src, size_t n)
{
    const size_t T = std::min<size_t>(4, n >> 23);
    if (T <= 1) {
        std::memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < T; t++)
        pool.emplace_back([=] { std::memcpy(dst + n * t / T, src + n * t / T, n * (t + 1) / T - n * t / T); });
    for (auto &th : pool)
        th.join();
}

/* a record ends with its fourth newline at the earliest: a short text with
 * fewer holds no complete record and need not go to the device (a request
 * that arrives in blocks of a few bytes) */
bool may_hold_record(const char *text, size_t n)
{
    if (n > 65536)
        return true;
    return std::count(text, text + n, '\n') >= 4;
}

}  // namespace

/* the fragment pass over reads where kgx_fq_parse left them, enqueued: what
 * upload_block does for reads the host parsed */
FqRequest::FqLaunched FqRequest::start_device(const kgx_fq_reads &reads, kgx_ctx *ctx)
{
    FqLaunched l;
    l.ctx = ctx;
    l.n_reads = reads.n_reads;
    if (l.n_reads == 0)
        return l;
    int rc = kgx_ctx_set_option(ctx, "fq_residues", 0);
    if (rc)
        throw_last(rc, "kgx_ctx_set_option");
    if ((rc = kgx_fq_fragments_device_start(ctx, reads.bases, reads.read_offsets, reads.n_reads, reads.n_bases)))
        throw_last(rc, "kgx_fq_fragments_device_start");
    return l;
}

/* process_text's rotation over the parts `next` hands out: part k + 2 is
 * framed on its context and its fragment pass enqueued while part k + 1's
 * lookup is launched and part k is collected.  One FamilyMapper for the
 * block. */
void FqRequest::run_device_parts(const std::function<bool(kgx_ctx *, DevicePart &)> &next, std::ostream &os)
{
    const bool timing = std::getenv("KGX_FQ_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    FamilyMapper mapper(kg_, mapping_);
    double device_ms = 0.0, frame_ms = 0.0;
    struct Slot {
        DevicePart p;
        FqLaunched l;
    } sl[3];
    size_t have = 0;
    bool last = false; /* `next` has no further part */
    auto prepare = [&]() {
        Slot &s = sl[have % 3];
        kgx_ctx *ctx = rotation_ctx(have % 3);
        s.p = DevicePart{};
        const auto p0 = std::chrono::steady_clock::now();
        if (!next(ctx, s.p)) {
            last = true;
            frame_ms += ms_since(p0);
            return;
        }
        s.l = s.p.host ? upload_block(s.p.host->view(), ctx) : start_device(s.p.reads, ctx);
        frame_ms += ms_since(p0);
        stats_.reads += s.l.n_reads;
        have++;
    };
    auto launch = [&](Slot &s) {
        const auto l0 = std::chrono::steady_clock::now();
        launch_uploaded(s.l);
        device_ms += ms_since(l0);
    };
    prepare();
    if (have)
        launch(sl[0]);
    if (!last)
        prepare();
    for (size_t k = 0; k < have; k++) {
        if (k + 1 < have) {
            if (!last)
                prepare();
            launch(sl[(k + 1) % 3]);
        }
        Slot &cur = sl[k % 3];
        FqBlock blk;
        if (cur.p.host) {
            blk = cur.p.host->view();
        } else {
            blk.n = cur.p.reads.n_reads;
            blk.device_reads = &cur.p.reads;
        }
        const auto f0 = std::chrono::steady_clock::now();
        finish_block(blk, cur.l, mapper, os);
        device_ms += ms_since(f0);
    }
    if (timing)
        std::fprintf(stderr, "[fq] block in %zu part(s), framed on the device: %.3f ms, framing %.3f ms, device + "
                             "frame choice %.3f ms\n",
                     have, ms_since(t0), frame_ms, device_ms);
}

void FqRequest::process_text_device(const char *text, size_t n, bool finished, std::ostream &os)
{
    DeviceBody &d = device_body();
    d.tail_to_host();
    d.parts.begin_block(n, fq_part_bytes());
    size_t pos = 0;
    bool rest_done = false;
    auto next = [&](kgx_ctx *ctx, DevicePart &out) -> bool {
        while (pos < n && !d.parts.beyond_limit(n - pos)) {
            const uint64_t kept = d.parts.have(), k = d.parts.take(n - pos);
            d.host_room((size_t)(kept + k), (size_t)kept);
            copy_bytes(d.part + kept, text + pos, (size_t)k);
            d.parts.took(k);
            pos += (size_t)k;
            const uint64_t have = d.parts.have();
            kgx_fq_reads r{};
            if (may_hold_record(d.part, (size_t)have)) {
                if (int rc = kgx_fq_parse(ctx, d.part, have, 0, &r))
                    throw_last(rc, "kgx_fq_parse");
                stats_.device_parts++;
            }
            if (r.consumed && have > r.consumed)
                std::memmove(d.part, d.part + r.consumed, (size_t)(have - r.consumed));
            d.parts.parsed(r.consumed, n - pos);
            stats_.tail_bytes_max = std::max(stats_.tail_bytes_max, d.parts.have());
            if (r.n_reads) {
                out.reads = r;
                return true;
            }
        }
        if (rest_done)
            return false;
        rest_done = true;
        /* a record too long for one parse: the rest of the block on the host;
         * the request's end: what the last complete record left */
        if (pos == n && !(finished && d.parts.have()))
            return false;
        const uint64_t kept = d.parts.have();
        d.host_room((size_t)(kept + (n - pos)), (size_t)kept);
        copy_bytes(d.part + kept, text + pos, n - pos);
        const size_t total = (size_t)kept + (n - pos);
        pos = n;
        stats_.host_parts++;
        out.host = d.host_rest(total, finished);
        return out.host != nullptr;
    };
    run_device_parts(next, os);
    if (finished)
        d.forget();
}

void FqRequest::process_members_device(bool finished, std::ostream &os)
{
    DeviceBody &d = device_body();
    GzipBodyReader &body = *body_;
    const std::vector<GzipListed> &list = body.list();
    const size_t n = list.size();
    std::vector<uint32_t> out_len(n);
    uint64_t text_bytes = 0;
    for (size_t i = 0; i < n; i++)
        text_bytes += out_len[i] = list[i].out_len;
    /* the compressed bytes go up once */
    d.device_room(&d.d_gz, &d.d_gz_cap, body.compressed_len());
    if (int rc = kgx_memcpy_h2d(d.d_gz, body.compressed(), body.compressed_len()))
        throw_last(rc, "kgx_memcpy_h2d");
    d.parts.begin_block(text_bytes, fq_part_bytes());
    size_t i = 0;
    bool rest_done = false, on_host = false;
    auto next = [&](kgx_ctx *ctx, DevicePart &out) -> bool {
        while (i < n) {
            uint64_t bytes = 0;
            const uint32_t k = d.parts.take_members(&out_len[i], (uint32_t)std::min<size_t>(n - i, UINT32_MAX), &bytes);
            if (d.parts.members_beyond_limit(bytes))
                break;
            /* the carry to the front of the other buffer, the members behind it */
            const uint64_t kept = d.parts.have();
            const int dst = d.cur ^ 1;
            void *q = d.d_text[dst];
            d.device_room(&q, &d.d_text_cap[dst], (size_t)(kept + bytes) + 16);
            d.d_text[dst] = static_cast<char *>(q);
            if (kept) {
                const int rc = d.tail_on_device
                                   ? kgx_ctx_memcpy_d2d(ctx, d.d_text[dst], d.d_text[d.cur] + d.tail_off, kept)
                                   : kgx_memcpy_h2d(d.d_text[dst], d.part, kept);
                if (rc)
                    throw_last(rc, "carried text");
            }
            if (int rc = body.inflate_listed(ctx, d.d_gz, (uint32_t)i, k, d.d_text[dst], kept))
                throw_last(rc, "kgx_gunzip");
            stats_.device_members += k;
            i += k;
            d.parts.took(bytes);
            d.cur = dst;
            d.tail_off = 0;
            d.tail_on_device = true;
            kgx_fq_reads r{};
            if (bytes) {
                if (int rc = kgx_fq_parse_device(ctx, d.d_text[dst], kept + bytes, 0, &r))
                    throw_last(rc, "kgx_fq_parse_device");
                stats_.device_parts++;
            }
            d.tail_off = r.consumed;
            d.parts.parsed(r.consumed, n - i);
            stats_.tail_bytes_max = std::max(stats_.tail_bytes_max, d.parts.have());
            if (r.n_reads) {
                out.reads = r;
                return true;
            }
        }
        if (rest_done)
            return false;
        rest_done = true;
        if (i == n && !(finished && d.parts.have()))
            return false;
        d.tail_to_host(); /* the one download of a request's carried text */
        const uint64_t kept = d.parts.have();
        size_t total = (size_t)kept;
        if (i < n) { /* a record too long for one parse: the block's members again, on the host */
            const uint64_t skip = list[i].out_off;
            const char *text = nullptr;
            size_t len = 0;
            on_host = true;
            if (int rc = body.inflate_listed_on_host(kg_.ctx(), finished, &text, &len))
                throw_last(rc, "kgx_gunzip");
            stats_.host_members += body.last_members();
            d.host_room((size_t)kept + (len - (size_t)skip), (size_t)kept);
            copy_bytes(d.part + kept, text + skip, len - (size_t)skip);
            total += len - (size_t)skip;
            i = n;
        }
        stats_.host_parts++;
        out.host = d.host_rest(total, finished);
        return out.host != nullptr;
    };
    run_device_parts(next, os);
    if (!on_host)
        body.listed_done(finished);
    if (finished)
        d.forget();
}

bool FqRequest::stat(const char *name, uint64_t *value) const
{
    const struct {
        const char *name;
        uint64_t v;
    } all[] = {{"device_parts", stats_.device_parts},     {"host_parts", stats_.host_parts},
               {"device_members", stats_.device_members}, {"host_members", stats_.host_members},
               {"ids_fetched", stats_.ids_fetched},       {"reads", stats_.reads},
               {"tail_bytes_max", stats_.tail_bytes_max}};
    for (const auto &s : all)
        if (!std::strcmp(s.name, name)) {
            *value = s.v;
            return true;
        }
    return false;
}

kgx_ctx *FqRequest::rotation_ctx(size_t i)
{
    if (i == 0)
        return kg_.ctx();
    kgx_ctx *&c = twin_[i - 1];
    if (!c) {
        int rc = kgx_ctx_create(kg_.image_->handle(), &c);
        if (rc)
            throw_last(rc, "kgx_ctx_create");
    }
    return c;
}

/* The block's parts (FqParts) rotate over three contexts, two parts ahead of
 * the one being collected: part k + 2's bases go up by DMA while part k + 1
 * is sized and its lookup enqueued and part k is collected, so the next probe
 * never waits for an upload (with two contexts and the upload inside the
 * launch, each part's 16-MB H2D ran with the GPU idle: 1.06 ms per part
 * against a 0.46-ms probe, r5j).  Parsing overlaps the device work and the
 * frame choice.  One FamilyMapper serves the whole block, as the reference
 * keeps one per block (fq_process_request.cc:241). */
void FqRequest::process_text(const char *text, size_t n, bool finished, std::ostream &os)
{
    const bool timing = std::getenv("KGX_FQ_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    FamilyMapper mapper(kg_, mapping_);
    double device_ms = 0.0;
    FqParts &src = *parts_;
    struct Slot {
        FqPart *pt = nullptr;
        FqLaunched l;
    } sl[3];
    size_t have = 0;   /* parts 0 .. have-1 are prepared (uploaded) */
    bool last = false; /* the last prepared part is the block's last */
    auto prepare = [&]() {
        Slot &s = sl[have % 3];
        s.pt = &src.get(have, have ? sl[(have - 1) % 3].pt : nullptr, &last);
        s.l = upload_block(s.pt->view(), rotation_ctx(have % 3));
        stats_.host_parts++;
        stats_.reads += s.l.n_reads;
        have++;
    };
    auto launch = [&](Slot &s) {
        const auto l0 = std::chrono::steady_clock::now();
        launch_uploaded(s.l);
        device_ms += ms_since(l0);
    };
    try {
        src.open(text, n, finished);
        prepare();
        launch(sl[0]);
        if (!last)
            prepare();
        for (size_t k = 0; k < have; k++) {
            if (k + 1 < have) {
                if (!last) /* part k + 2 up while k + 1 launches and k finishes */
                    prepare();
                launch(sl[(k + 1) % 3]);
            }
            Slot &cur = sl[k % 3];
            const auto f0 = std::chrono::steady_clock::now();
            finish_block(cur.pt->view(), cur.l, mapper, os);
            device_ms += ms_since(f0);
            src.release(k);
        }
    } catch (...) {
        src.close();
        throw;
    }
    src.close();
    if (timing)
        std::fprintf(stderr, "[fq] block %.1f MB in %zu part(s): %.3f ms, waiting for the parse %.3f ms, device + "
                             "frame choice %.3f ms\n",
                     n / 1e6, src.planned(), ms_since(t0), src.wait_ms, device_ms);
}

void FqRequest::process_reads(const std::vector<std::pair<std::string, std::string>> &reads, std::ostream &os)
{
    size_t nb = 0;
    for (auto &r : reads)
        nb += r.second.size();
    FqPart pt;
    pt.begin(nb, FQ_START, std::string(), nullptr, 0);
    for (auto &r : reads) {
        pt.id_chars += r.first;
        pt.id_off.push_back(pt.id_chars.size());
        std::memcpy(pt.bases + pt.len, r.second.data(), r.second.size());
        pt.len += r.second.size();
        pt.roff.push_back(pt.len);
    }
    FamilyMapper mapper(kg_, mapping_);
    stats_.host_parts++;
    stats_.reads += reads.size();
    process_block(pt.view(), mapper, os);
}

void FqRequest::process_block(const FqBlock &blk, FamilyMapper &mapper, std::ostream &os)
{
    FqLaunched l = launch_block(blk, kg_.ctx());
    finish_block(blk, l, mapper, os);
}

FqRequest::FqLaunched FqRequest::upload_block(const FqBlock &blk, kgx_ctx *ctx)
{
    FqLaunched l;
    l.ctx = ctx;
    l.n_reads = (uint32_t)blk.n_reads();
    if (l.n_reads == 0)
        return l;
    int rc = kgx_fq_upload(ctx, blk.residues(), blk.roff, l.n_reads);
    if (rc)
        throw_last(rc, "kgx_fq_upload");
    /* fragments as anchors into the bases: the probe translates their windows
     * itself and no residue goes through HBM (the context keeps residues when
     * its probe cannot take anchors) */
    if ((rc = kgx_ctx_set_option(ctx, "fq_residues", 0)))
        throw_last(rc, "kgx_ctx_set_option");
    if ((rc = kgx_fq_fragments_uploaded_start(ctx)))
        throw_last(rc, "kgx_fq_fragments_uploaded_start");
    return l;
}

void FqRequest::launch_uploaded(FqLaunched &l)
{
    if (l.n_reads == 0)
        return;
    kgx_ctx *ctx = l.ctx;
    int rc = kgx_fq_fragments_finish(ctx, &l.fr); /* the pass upload_block enqueued */
    if (rc)
        throw_last(rc, "kgx_fq_fragments_finish");
    kgx_params p{kg_.min_hits, kg_.max_gap, kg_.order_constraint, kg_.min_weighted_hits};
    /* Calls are sparse over fragments (most fragments of a read are noise),
     * so the calls come back and find_best_call runs on the host for the
     * fragments that have any: a per-fragment device decision (KGX_WANT_BEST)
     * would copy 24 B for every fragment (measured: 8.3M -> 6.7M reads/s).
     * The hits stay on the device for the rollups. */
    rc = kgx_fq_run_device(ctx, &p, &l.fr, KGX_WANT_CALLS, nullptr);
    if (rc)
        throw_last(rc, "kgx_fq_run_device");
}

/* the block's reads -> fragments -> lookup, one GPU batch on ctx: returns
 * once the fragment pass has sized the batch and the lookup is enqueued */
FqRequest::FqLaunched FqRequest::launch_block(const FqBlock &blk, kgx_ctx *ctx)
{
    FqLaunched l = upload_block(blk, ctx);
    launch_uploaded(l);
    return l;
}

namespace {

/* a block's fragments as choose_frame reads them */
struct FrameView {
    const uint64_t *call_offsets; /* fragment g's calls: calls[call_offsets[g], call_offsets[g + 1]) */
    const kgx_call *calls;
    const uint64_t *row_offsets; /* its on_hit rollups likewise; null without family lists */
    const kgx_rollup_row *rows;
    /* its length, printed with a match: frag_len[g], or from the fragments'
     * offsets -- all on the host, or (null) a printed read's slice fetched
     * from the device */
    const uint32_t *frag_len;
    const uint64_t *offsets, *d_offsets;
};

/* what choose_frame keeps across a block's reads (buffers reused) */
struct FrameScratch {
    std::vector<KmerCall> calls;
    std::vector<FamilyMapper::best_match_t> matches, best_matches;
    std::vector<uint64_t> match_frag, best_frag, slice;
};

/* on_parsed_seq (fq_process_request.cc:298-365) for one read: its fragments
 * start at g, frame_counts[0..5] of them in frame slots 1, 2, 3, -1, -2, -3;
 * each fragment's calls and rollups go through the block's FamilyMapper in
 * order, the frame with the best running score wins, and a read that scores
 * writes its line */
void choose_frame(const FrameView &v, uint64_t g, const uint32_t *frame_counts, const char *id, size_t id_len,
                  FamilyMapper &mapper, FrameScratch &s, std::ostream &os)
{
    const uint64_t g0 = g;
    double best_score = 0.0;
    int best_frame = 0;
    s.best_matches.clear();
    s.best_frag.clear();
    for (int fs = 0; fs < 6; fs++) {
        const int frame = fs < 3 ? fs + 1 : -(fs - 2);
        const uint64_t g_end = g + frame_counts[fs];
        double score = 0.0;
        s.matches.clear();
        s.match_frag.clear();
        for (; g < g_end; g++) {
            s.calls.clear();
            for (uint64_t c = v.call_offsets[g]; c < v.call_offsets[g + 1]; c++)
                s.calls.emplace_back(v.calls[c].start, v.calls[c].end, v.calls[c].count, v.calls[c].function_index,
                                     v.calls[c].weighted_hits);
            const uint64_t r0 = v.row_offsets ? v.row_offsets[g] : 0, r1 = v.row_offsets ? v.row_offsets[g + 1] : 0;
            s.matches.push_back(mapper.find_best_family_match(v.row_offsets ? v.rows + r0 : nullptr, r1 - r0, s.calls));
            s.match_frag.push_back(g);
            score += s.matches.back().score;
            if (score > best_score) {
                best_score = score;
                best_frame = frame;
                s.best_matches = s.matches;
                s.best_frag = s.match_frag;
            }
        }
    }
    if (best_score <= 0.0)
        return;
    const uint64_t *offs = v.offsets;
    if (!v.frag_len && !offs) {
        s.slice.resize(g - g0 + 1);
        if (int rc = kgx_memcpy_d2h(s.slice.data(), v.d_offsets + g0, s.slice.size() * 8))
            throw_last(rc, "fragment offsets");
        offs = s.slice.data() - g0;
    }
    os.write(id, (std::streamsize)id_len);
    os << "\t" << best_frame << "\t" << best_score << "\t";
    for (size_t i = 0; i < s.best_matches.size(); i++) {
        const uint64_t f = s.best_frag[i];
        if (i)
            os << "\t";
        os << (size_t)(v.frag_len ? v.frag_len[f] : offs[f + 1] - offs[f]) << "\t" << s.best_matches[i];
    }
    os << std::endl;
}

}  // namespace

void FqRequest::finish_block(const FqBlock &blk, FqLaunched &l, FamilyMapper &mapper, std::ostream &os)
{
    const uint32_t n_reads = l.n_reads;
    if (n_reads == 0)
        return;
    /* KGX_FQ_TIMING=2: per-phase wall times on stderr */
    static const bool timing = std::getenv("KGX_FQ_TIMING") != nullptr && std::getenv("KGX_FQ_TIMING")[0] == '2';
    auto t_last = std::chrono::steady_clock::now();
    kgx_ctx *ctx = l.ctx;
    auto mark = [&](const char *what) {
        if (!timing)
            return;
        kgx_ctx_synchronize(ctx);
        std::fprintf(stderr, "[fq] %-12s %8.3f ms\n", what, ms_since(t_last));
        t_last = std::chrono::steady_clock::now();
    };
    kgx_fragments &fr = l.fr;
    int rc;
    FrameScratch scratch;
    /* Without family lists a fragment's match depends on its calls alone,
     * and a read without calls scores 0 in every frame: no output and no
     * FamilyMapper state (seq_score_ stays empty).  Only then may reads
     * without calls be skipped and hits stay on the device; with families
     * loaded every fragment is replayed, since each one grows seq_score_ and
     * so shapes the iteration order later reads see. */
    const bool families = kgx_kmap_num_kmers(mapping_->kmer_to_family_id()) > 0;
    mark("lookup");
    if (!families) {
        /* only the reads with a call in some fragment come back (sparse):
         * the others produce no output and no mapper state */
        kgx_fq_called cr;
        if ((rc = kgx_fq_called_reads(ctx, &fr, &cr)))
            throw_last(rc, "kgx_fq_called_reads");
        mark("collect");
        const FrameView view{cr.call_offsets, cr.calls, nullptr, nullptr, cr.frag_len, nullptr, nullptr};
        /* a device-framed part: the ids of these reads alone come down, in their order */
        FqBlock ids = blk;
        if (blk.device_reads) {
            kgx_fq_ids got;
            if ((rc = kgx_fq_read_ids(ctx, blk.device_reads, cr.reads, cr.n, &got)))
                throw_last(rc, "kgx_fq_read_ids");
            stats_.ids_fetched += cr.n;
            ids.ids = got.ids;
            ids.id_off = got.id_offsets;
        }
        for (uint32_t i = 0; i < cr.n; i++) {
            const size_t r = blk.device_reads ? i : cr.reads[i];
            if (ids.id_len(r))
                choose_frame(view, cr.frag_offsets[i], cr.frame_counts + (size_t)i * 6, ids.id(r), ids.id_len(r), mapper,
                             scratch, os);
        }
        mark("host loop");
        return;
    }
    /* every read with an id is replayed: a device-framed part's ids all come down */
    FqBlock ids = blk;
    if (blk.device_reads) {
        std::vector<uint32_t> all(n_reads);
        std::iota(all.begin(), all.end(), 0u);
        kgx_fq_ids got;
        if ((rc = kgx_fq_read_ids(ctx, blk.device_reads, all.data(), n_reads, &got)))
            throw_last(rc, "kgx_fq_read_ids");
        stats_.ids_fetched += n_reads;
        ids.ids = got.ids;
        ids.id_off = got.id_offsets;
    }
    /* fragments per (read, frame): fragment g of read r, frame slot k */
    std::vector<uint32_t> fcount((size_t)n_reads * 6);
    if ((rc = kgx_ctx_synchronize(ctx)) || (rc = kgx_memcpy_d2h(fcount.data(), fr.frame_counts, fcount.size() * 4)))
        throw_last(rc, "fragment counts");
    kgx_result res;
    rc = kgx_device_batch_collect(ctx, KGX_WANT_CALLS, &res);
    if (rc)
        throw_last(rc, "kgx_device_batch_collect");
    mark("collect");
    /* on_hit's rollups of every fragment (family_mapper.cc:287-312) on the device */
    kgx_rollup_result ru;
    if ((rc = kgx_kmap_rollup(mapping_->kmer_to_family_id(), ctx, KGX_ROLLUP_FAMILY, &ru)))
        throw_last(rc, "kgx_kmap_rollup");
    /* fragment lengths (printed for matches) are needed only for reads with
     * calls: fetch their offset slices, or all offsets when there are many */
    std::vector<uint64_t> rfirst(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) {
        uint64_t k = 0;
        for (int f = 0; f < 6; f++)
            k += fcount[(size_t)r * 6 + f];
        rfirst[r + 1] = rfirst[r] + k;
    }
    size_t n_called = 0;
    for (uint32_t r = 0; r < n_reads; r++)
        n_called += res.call_offsets[rfirst[r + 1]] != res.call_offsets[rfirst[r]];
    std::vector<uint64_t> frag_off;
    if (n_called > 1024) {
        frag_off.resize(fr.n_fragments + 1);
        if ((rc = kgx_memcpy_d2h(frag_off.data(), fr.offsets, frag_off.size() * 8)))
            throw_last(rc, "fragment offsets");
    }
    mark("family lists");
    const FrameView view{res.call_offsets, res.calls, ru.offsets, ru.rows, nullptr,
                         frag_off.empty() ? nullptr : frag_off.data(), fr.offsets};
    /* reads in order, every one with an id */
    for (uint32_t r = 0; r < n_reads; r++)
        if (ids.id_len(r))
            choose_frame(view, rfirst[r], &fcount[(size_t)r * 6], ids.id(r), ids.id_len(r), mapper, scratch, os);
    mark("host loop");
}

}  // namespace kgx

/* ---- C ABI of the fq request handler (include/kgx.h kgx_fq_*) ------------- */

struct kgx_fq {
    std::unique_ptr<kgx::KmerGuts> kg;
    std::shared_ptr<kgx::KmerPegMapping> mapping;
    std::unique_ptr<kgx::FqRequest> req;
    std::string text;
};

extern "C" {

int kgx_fq_create(kgx_image *img, const char *data_dir, const char *genus_file, const char *families_file,
                  const char *nr_fasta, kgx_fq **out)
{
    if (!img || !data_dir || !out)
        return kgx::fail(KGX_EINVAL, "null argument");
    kgx_fq *q = new kgx_fq;
    try {
        auto image = std::make_shared<kgx::KmerImage>(img, false);
        q->kg.reset(new kgx::KmerGuts(data_dir, image));
        q->mapping = std::make_shared<kgx::KmerPegMapping>(kgx_image_device(img));
        if (genus_file && *genus_file)
            q->mapping->load_genus_map(genus_file);
        if (families_file && *families_file)
            q->mapping->load_families(families_file);
        if (nr_fasta && *nr_fasta)
            q->mapping->load_nr_families(*q->kg, nr_fasta);
        q->req.reset(new kgx::FqRequest(*q->kg, q->mapping));
    } catch (const kgx::Error &e) {
        delete q;
        return kgx::fail(e.code(), e.what());
    } catch (const std::exception &e) {
        delete q;
        return kgx::fail(KGX_EINVAL, e.what());
    }
    *out = q;
    return KGX_OK;
}

int kgx_fq_destroy(kgx_fq *q)
{
    delete q;
    return KGX_OK;
}

int kgx_fq_stat(kgx_fq *q, const char *name, uint64_t *value)
{
    if (!q || !name || !value)
        return kgx::fail(KGX_EINVAL, "null argument");
    if (!q->req->stat(name, value))
        return kgx::fail(KGX_EINVAL, std::string("unknown statistic ") + name);
    return KGX_OK;
}

int kgx_fq_process(kgx_fq *q, const char *fastq, uint64_t n, int finished, const char **text, uint64_t *text_len)
{
    if (!q || (n && !fastq) || !text || !text_len)
        return kgx::fail(KGX_EINVAL, "null argument");
    try {
        std::ostringstream os;
        q->req->process(fastq ? fastq : "", (size_t)n, finished != 0, os);
        q->text = os.str();
    } catch (const kgx::Error &e) {
        return kgx::fail(e.code(), e.what());
    } catch (const std::exception &e) {
        return kgx::fail(KGX_EINVAL, e.what());
    }
    *text = q->text.data();
    *text_len = q->text.size();
    return KGX_OK;
}

}  // extern "C"
