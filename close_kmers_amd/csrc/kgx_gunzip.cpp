/*
 * kgx_gunzip.cpp -- the gzip entry points of the C ABI (include/kgx.h):
 * the framing walk over a body's members (kgx_gzip.h), blocked members
 * through the device kernel (kgx_inflate.hip) or over host threads, plain
 * members on the calling thread.  One decoder source for all of them
 * (kgx_inflate.h); no zlib.  Over them, GzipBodyReader: the text-or-gzip
 * front end of the fq handler and of fastq_to_protein.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <thread>
#include <vector>

#include "kgx_gzip.h"
#include "kgx_rt.h"

using namespace kgx;

static_assert(sizeof(kgx_inflate_stats) == sizeof(InflateStats), "kgx_inflate_stats mirrors InflateStats");
static_assert(sizeof(kgx_gz_member) == 32 && sizeof(kgx_gz_status) == 16, "device records");

namespace {

constexpr unsigned HOST_THREADS_MAX = 16;

struct Blocked {
    uint64_t index; /* the member's number in the body */
    kgx_gz_member m;
};

std::string member_error(uint64_t index, uint32_t reason, uint64_t bit_pos)
{
    return "gunzip: member " + std::to_string(index) + ": " + gzip_reason_text(reason) + " (reason " +
           std::to_string(reason) + ") at bit " + std::to_string(bit_pos);
}

void add_stats(kgx_inflate_stats &sum, const kgx_inflate_stats &s)
{
    sum.stored_blocks += s.stored_blocks;
    sum.fixed_blocks += s.fixed_blocks;
    sum.dynamic_blocks += s.dynamic_blocks;
    sum.matches += s.matches;
    sum.max_code_len = std::max(sum.max_code_len, s.max_code_len);
    sum.max_distance = std::max(sum.max_distance, s.max_distance);
    sum.max_length = std::max(sum.max_length, s.max_length);
    sum.overlap |= s.overlap;
}

kgx_inflate_stats to_abi(const InflateStats &s)
{
    return kgx_inflate_stats{s.stored_blocks, s.fixed_blocks, s.dynamic_blocks, s.max_code_len,
                             s.max_distance,  s.max_length,   s.overlap,        s.matches};
}

/* gzip_blocked_extent as the kernel's record (offsets relative to p) */
int blocked_member(const uint8_t *p, uint64_t n, const GzipHeader &h, kgx_gz_member *m)
{
    GzipBlocked b;
    const int r = gzip_blocked_extent(p, n, h, &b);
    if (r == 0)
        *m = kgx_gz_member{h.header_len, 0, b.data_len, b.isize, b.crc, 0};
    return r;
}

/* blocked members on host threads, each into its slot of out */
void inflate_blocked_host(const uint8_t *gz, const std::vector<Blocked> &v, uint8_t *out, kgx_gz_status *status,
                          kgx_inflate_stats *stats)
{
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned T = (unsigned)std::min<size_t>(std::min(hw, HOST_THREADS_MAX), v.size());
    auto work = [&](unsigned t) {
        InflateTables tables;
        for (size_t i = t; i < v.size(); i += T) {
            const kgx_gz_member &m = v[i].m;
            InflateStats st;
            const InflateResult r = gzip_member_inflate(gz + m.in_off, gz + m.in_off + m.in_len, true,
                                                        out + m.out_off, m.out_len, &tables, &st, nullptr);
            status[i] = kgx_gz_status{r.reason, (uint32_t)r.out_len, r.bit_pos};
            stats[i] = to_abi(st);
        }
    };
    if (T <= 1) {
        work(0);
        return;
    }
    std::vector<std::thread> ths;
    for (unsigned t = 0; t < T; t++)
        ths.emplace_back(work, t);
    for (auto &th : ths)
        th.join();
}

int ensure_gz_events(kgx_ctx *c) { return ensure_events(c->gz_events, 4, hipEventDefault); }

/* members through the kernel: d_gz / d_out are the bases the members' offsets
 * count from; status and stats come back into the context's pinned arrays */
int run_kernel(kgx_ctx *c, const uint8_t *d_gz, const kgx_gz_member *members, uint32_t n, uint8_t *d_out)
{
    HIP_TRY(c->gz_members.reserve((size_t)n * sizeof(kgx_gz_member)));
    HIP_TRY(c->gz_status.reserve((size_t)n * sizeof(kgx_gz_status)));
    HIP_TRY(c->gz_stats.reserve((size_t)n * sizeof(kgx_inflate_stats)));
    HIP_TRY(c->h_gz_members.resize(n));
    HIP_TRY(c->h_gz_status.resize(n));
    HIP_TRY(c->h_gz_stats.resize(n));
    std::copy(members, members + n, c->h_gz_members.data());
    HIP_TRY(hipMemcpyAsync(c->gz_members.p, c->h_gz_members.data(), (size_t)n * sizeof(kgx_gz_member),
                           hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->gz_events[1], c->stream));
    HIP_TRY(launch_inflate_members(d_gz, c->gz_members.as<kgx_gz_member>(), n, d_out, c->gz_status.as<kgx_gz_status>(),
                                   c->gz_stats.as<kgx_inflate_stats>(), c->stream));
    HIP_TRY(hipEventRecord(c->gz_events[2], c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_gz_status.data(), c->gz_status.p, (size_t)n * sizeof(kgx_gz_status),
                           hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(c->h_gz_stats.data(), c->gz_stats.p, (size_t)n * sizeof(kgx_inflate_stats),
                           hipMemcpyDeviceToHost, c->stream));
    return KGX_OK;
}

}  // namespace

extern "C" {

int kgx_inflate_host(const void *gz, uint64_t n, void *out, uint64_t cap, uint64_t *out_len, uint64_t *in_used,
                     kgx_inflate_stats *stats, uint32_t *reason, uint64_t *bit_pos)
{
    if ((n && !gz) || (cap && !out))
        return fail(KGX_EINVAL, "null argument");
    static const uint8_t none = 0;
    static uint8_t sink = 0;
    const uint8_t *in = gz ? static_cast<const uint8_t *>(gz) : &none;
    uint8_t *o = out ? static_cast<uint8_t *>(out) : &sink;
    InflateTables tables;
    InflateStats st;
    HostIO io;
    const InflateResult r = inflate_raw(in, in + n, o, o + cap, &tables, &st, io);
    if (out_len)
        *out_len = r.out_len;
    if (in_used)
        *in_used = (r.bit_pos + 7) / 8;
    if (stats)
        *stats = to_abi(st);
    if (reason)
        *reason = r.reason;
    if (bit_pos)
        *bit_pos = r.bit_pos;
    if (r.reason)
        return fail(KGX_EFORMAT, std::string("inflate: ") + inflate_reason_text(r.reason) + " (reason " +
                                     std::to_string(r.reason) + ") at bit " + std::to_string(r.bit_pos));
    return KGX_OK;
}

int kgx_gunzip_scan(const void *gz, uint64_t n, int finished, uint64_t *members, uint64_t *blocked,
                    uint64_t *out_bytes, uint64_t *consumed)
{
    if (n && !gz)
        return fail(KGX_EINVAL, "null argument");
    const uint8_t *p = static_cast<const uint8_t *>(gz);
    uint64_t pos = 0, nb = 0, nm = 0, ob = 0;
    while (pos < n) {
        GzipHeader h;
        uint32_t reason = 0;
        const int hr = gzip_header(p + pos, n - pos, &h, &reason);
        if (hr == GZ_HDR_BAD) {
            if (reason == GZ_NOT_GZIP && nb) { /* trailing garbage */
                pos = n;
                break;
            }
            return fail(KGX_EFORMAT, member_error(nb, reason, 0));
        }
        if (hr == GZ_HDR_MORE) {
            if (finished)
                return fail(KGX_EFORMAT, member_error(nb, GZ_TRUNCATED, 0));
            break;
        }
        if (!h.blocked) {
            nm = 1;
            break;
        }
        kgx_gz_member m;
        const int br = blocked_member(p + pos, n - pos, h, &m);
        if (br == 1) {
            if (finished)
                return fail(KGX_EFORMAT, member_error(nb, GZ_TRUNCATED, 0));
            break;
        }
        if (br)
            return fail(KGX_EFORMAT, member_error(nb, (uint32_t)br - 2, 0));
        pos += (uint64_t)h.bsize + 1;
        ob += m.out_len;
        nb++;
    }
    if (members)
        *members = nb + nm;
    if (blocked)
        *blocked = nb;
    if (out_bytes)
        *out_bytes = ob;
    if (consumed)
        *consumed = pos;
    return KGX_OK;
}

int kgx_gunzip_device(kgx_ctx *c, const void *d_gz, const kgx_gz_member *members, uint32_t n_members, void *d_out,
                      kgx_gz_status *status, kgx_inflate_stats *member_stats, float *kernel_ms)
{
    if (!c || !status || (n_members && (!d_gz || !members || !d_out)))
        return fail(KGX_EINVAL, "null argument");
    if (kernel_ms)
        *kernel_ms = 0.0f;
    if (n_members == 0)
        return KGX_OK;
    HIP_TRY(hipSetDevice(c->img->device));
    if (int rc = ensure_gz_events(c))
        return rc;
    if (int rc = run_kernel(c, static_cast<const uint8_t *>(d_gz), members, n_members, static_cast<uint8_t *>(d_out)))
        return rc;
    HIP_TRY(host_wait(c->stream));
    if (kernel_ms)
        HIP_TRY(hipEventElapsedTime(kernel_ms, c->gz_events[1], c->gz_events[2]));
    std::copy(c->h_gz_status.data(), c->h_gz_status.data() + n_members, status);
    if (member_stats)
        std::copy(c->h_gz_stats.data(), c->h_gz_stats.data() + n_members, member_stats);
    for (uint32_t i = 0; i < n_members; i++)
        if (status[i].reason)
            return fail(KGX_EFORMAT, member_error(i, status[i].reason, status[i].bit_pos));
    return KGX_OK;
}

int kgx_gunzip(kgx_ctx *c, const void *gz, uint64_t n, int finished, void *out, uint64_t cap, uint64_t *out_len,
               uint64_t *consumed, kgx_gunzip_stats *stats)
{
    if ((n && !gz) || (cap && !out) || !out_len || !consumed)
        return fail(KGX_EINVAL, "null argument");
    const uint8_t *p = static_cast<const uint8_t *>(gz);
    uint8_t *o = static_cast<uint8_t *>(out);
    kgx_gunzip_stats gs{};
    *out_len = 0;
    *consumed = 0;
    std::vector<Blocked> blocked;
    uint64_t pos = 0, opos = 0, index = 0;
    while (pos < n) {
        GzipHeader h;
        uint32_t reason = 0;
        const int hr = gzip_header(p + pos, n - pos, &h, &reason);
        if (hr == GZ_HDR_BAD) {
            if (reason == GZ_NOT_GZIP && index) { /* trailing garbage */
                pos = n;
                break;
            }
            return fail(KGX_EFORMAT, member_error(index, reason, 0));
        }
        if (hr == GZ_HDR_MORE) {
            if (finished)
                return fail(KGX_EFORMAT, member_error(index, GZ_TRUNCATED, 0));
            break;
        }
        if (h.blocked) {
            kgx_gz_member m;
            const int br = blocked_member(p + pos, n - pos, h, &m);
            if (br == 1) {
                if (finished)
                    return fail(KGX_EFORMAT, member_error(index, GZ_TRUNCATED, 0));
                break;
            }
            if (br)
                return fail(KGX_EFORMAT, member_error(index, (uint32_t)br - 2, 0));
            if (m.out_len > cap - opos)
                return fail(KGX_ERANGE, "gunzip: the output needs more than " + std::to_string(cap) + " bytes");
            m.in_off += pos;
            m.out_off = opos;
            blocked.push_back(Blocked{index, m});
            pos += (uint64_t)h.bsize + 1;
            opos += m.out_len;
        } else {
            if (!finished) /* its end is known only by decoding it whole */
                break;
            InflateTables tables;
            InflateStats st;
            const uint8_t *end = nullptr;
            const InflateResult r = gzip_member_inflate(p + pos + h.header_len, p + n, false, o + opos, cap - opos,
                                                        &tables, &st, &end);
            if (r.reason == INF_OUTPUT_FULL && !r.trailer) /* the room, not ISIZE */
                return fail(KGX_ERANGE, "gunzip: the output needs more than " + std::to_string(cap) + " bytes");
            if (r.reason)
                return fail(KGX_EFORMAT, member_error(index, r.reason == INF_INPUT_END ? (uint32_t)GZ_TRUNCATED : r.reason,
                                                      r.bit_pos));
            add_stats(gs.inflate, to_abi(st));
            gs.plain_members++;
            pos = (uint64_t)(end - p);
            opos += r.out_len;
        }
        index++;
    }
    gs.members = index;
    gs.bytes_in = pos;
    gs.bytes_out = opos;
    if (!blocked.empty()) {
        const size_t nb = blocked.size();
        const bool device = c && c->opt.gunzip_device;
        std::vector<kgx_gz_status> h_status;
        std::vector<kgx_inflate_stats> h_stats;
        const kgx_gz_status *status = nullptr;
        const kgx_inflate_stats *mstats = nullptr;
        if (!device) {
            h_status.resize(nb);
            h_stats.resize(nb);
            inflate_blocked_host(p, blocked, o, h_status.data(), h_stats.data());
            status = h_status.data();
            mstats = h_stats.data();
            gs.host_blocked_members = nb;
        } else {
            if (nb > UINT32_MAX)
                return fail(KGX_ERANGE, "gunzip: more than 2^32 members in one call");
            HIP_TRY(hipSetDevice(c->img->device));
            if (int rc = ensure_gz_events(c))
                return rc;
            /* the span of compressed bytes and of output the blocked members cover */
            const uint64_t in_lo = blocked.front().m.in_off, in_hi = blocked.back().m.in_off + blocked.back().m.in_len;
            const uint64_t out_lo = blocked.front().m.out_off,
                           out_hi = blocked.back().m.out_off + blocked.back().m.out_len;
            HIP_TRY(c->gz_in.reserve(in_hi - in_lo));
            HIP_TRY(c->gz_out.reserve(std::max<uint64_t>(out_hi - out_lo, 1)));
            std::vector<kgx_gz_member> rel(nb);
            for (size_t i = 0; i < nb; i++) {
                rel[i] = blocked[i].m;
                rel[i].in_off -= in_lo;
                rel[i].out_off -= out_lo;
            }
            HIP_TRY(hipEventRecord(c->gz_events[0], c->stream));
            HIP_TRY(hipMemcpyAsync(c->gz_in.p, p + in_lo, in_hi - in_lo, hipMemcpyHostToDevice, c->stream));
            if (int rc = run_kernel(c, c->gz_in.as<uint8_t>(), rel.data(), (uint32_t)nb, c->gz_out.as<uint8_t>()))
                return rc;
            /* down in runs of adjacent slots: a plain member's text between
             * two blocked ones is already in out */
            for (size_t i = 0; i < nb;) {
                size_t j = i + 1;
                while (j < nb && blocked[j].m.out_off == blocked[j - 1].m.out_off + blocked[j - 1].m.out_len &&
                       blocked[j].index == blocked[j - 1].index + 1)
                    j++;
                const uint64_t a = blocked[i].m.out_off, b = blocked[j - 1].m.out_off + blocked[j - 1].m.out_len;
                if (b > a)
                    HIP_TRY(hipMemcpyAsync(o + a, c->gz_out.as<uint8_t>() + (a - out_lo), b - a, hipMemcpyDeviceToHost,
                                           c->stream));
                i = j;
            }
            HIP_TRY(hipEventRecord(c->gz_events[3], c->stream));
            HIP_TRY(host_wait(c->stream));
            HIP_TRY(hipEventElapsedTime(&gs.upload_ms, c->gz_events[0], c->gz_events[1]));
            HIP_TRY(hipEventElapsedTime(&gs.kernel_ms, c->gz_events[1], c->gz_events[2]));
            HIP_TRY(hipEventElapsedTime(&gs.download_ms, c->gz_events[2], c->gz_events[3]));
            status = c->h_gz_status.data();
            mstats = c->h_gz_stats.data();
            gs.device_members = nb;
        }
        for (size_t i = 0; i < nb; i++) {
            if (status[i].reason)
                return fail(KGX_EFORMAT, member_error(blocked[i].index, status[i].reason, status[i].bit_pos));
            add_stats(gs.inflate, mstats[i]);
        }
    }
    *out_len = opos;
    *consumed = pos;
    if (stats)
        *stats = gs;
    return KGX_OK;
}

}  // extern "C"

/* ---- GzipBodyReader (kgx_gzip.h), over the entry points above ------------- */

namespace kgx {

GzipBodyReader::~GzipBodyReader()
{
    if (text_)
        kgx_host_free(text_);
}

void GzipBodyReader::reset()
{
    body_ = GZ_BODY_UNKNOWN;
    tail_.clear();
    members_ = 0;
}

int GzipBodyReader::feed(kgx_ctx *ctx, const char *block, size_t n, bool finished, bool fresh, const char **text,
                         size_t *len)
{
    return feed_listed(ctx, block, n, finished, fresh, text, len, nullptr);
}

/* the complete members at the front of tail_, when all of them are blocked:
 * list_ and list_len_ (empty: a plain member is among them, or there is none) */
int GzipBodyReader::list_blocked(bool finished)
{
    list_.clear();
    list_len_ = 0;
    if (members_ && tail_.size() >= 2 && !((unsigned char)tail_[0] == 0x1f && (unsigned char)tail_[1] == 0x8b))
        tail_.clear(); /* trailing bytes that are no gzip */
    uint64_t members = 0, blocked = 0, out_bytes = 0, consumed = 0;
    if (int rc = kgx_gunzip_scan(tail_.data(), tail_.size(), finished, &members, &blocked, &out_bytes, &consumed))
        return rc;
    if (members != blocked || !blocked)
        return KGX_OK;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(tail_.data());
    uint64_t pos = 0, opos = 0;
    for (uint64_t i = 0; i < blocked; i++) { /* the walk kgx_gunzip_scan has just made */
        GzipHeader h;
        uint32_t reason = 0;
        GzipBlocked b;
        if (gzip_header(p + pos, tail_.size() - pos, &h, &reason) != GZ_HDR_OK ||
            gzip_blocked_extent(p + pos, tail_.size() - pos, h, &b) != 0)
            return fail(KGX_EFORMAT, member_error(i, reason ? reason : (uint32_t)GZ_TRUNCATED, 0));
        list_.push_back(GzipListed{pos + h.header_len, opos, b.data_len, b.isize, b.crc});
        pos += b.total;
        opos += b.isize;
    }
    list_len_ = (size_t)consumed; /* trailing bytes that are no gzip included */
    return KGX_OK;
}

int GzipBodyReader::inflate_listed(kgx_ctx *ctx, const void *d_gz, uint32_t first, uint32_t count, void *d_out,
                                   uint64_t out_base)
{
    if (!ctx || (uint64_t)first + count > list_.size() || (count && (!d_gz || !d_out)))
        return fail(KGX_EINVAL, "inflate_listed: bad argument");
    if (!count)
        return KGX_OK;
    HIP_TRY(hipSetDevice(ctx->img->device));
    if (int rc = ensure_gz_events(ctx))
        return rc;
    std::vector<kgx_gz_member> m(count);
    for (uint32_t i = 0; i < count; i++) {
        const GzipListed &l = list_[first + i];
        m[i] = kgx_gz_member{l.in_off, out_base + (l.out_off - list_[first].out_off), l.in_len, l.out_len, l.crc, 0};
    }
    if (int rc = run_kernel(ctx, static_cast<const uint8_t *>(d_gz), m.data(), count, static_cast<uint8_t *>(d_out)))
        return rc;
    HIP_TRY(host_wait(ctx->stream));
    for (uint32_t i = 0; i < count; i++)
        if (ctx->h_gz_status[i].reason)
            return fail(KGX_EFORMAT,
                        member_error((uint64_t)first + i, ctx->h_gz_status[i].reason, ctx->h_gz_status[i].bit_pos));
    return KGX_OK;
}

void GzipBodyReader::listed_done(bool finished)
{
    members_ += list_.size();
    tail_.erase(0, list_len_);
    list_.clear();
    list_len_ = 0;
    if (finished)
        reset();
}

int GzipBodyReader::inflate_listed_on_host(kgx_ctx *ctx, bool finished, const char **text, size_t *len)
{
    list_.clear();
    list_len_ = 0;
    const int rc = inflate(ctx, finished, len);
    *text = text_;
    if (rc || finished)
        reset();
    return rc;
}

int GzipBodyReader::feed_listed(kgx_ctx *ctx, const char *block, size_t n, bool finished, bool fresh,
                                const char **text, size_t *len, bool *listed)
{
    *text = nullptr;
    *len = 0;
    last_members_ = 0;
    if (listed)
        *listed = false;
    bool joined = false;
    if (body_ == GZ_BODY_UNKNOWN || body_ == GZ_BODY_HELD) {
        body_ = gzip_sniff(tail_.data(), tail_.size(), block, n, finished, fresh);
        if (body_ == GZ_BODY_HELD) {
            tail_.append(block, n);
            return KGX_OK;
        }
        joined = body_ == GZ_BODY_TEXT && !tail_.empty();
    }
    gzip_ = body_ == GZ_BODY_GZIP;
    int rc = KGX_OK;
    if (gzip_) {
        tail_.append(block, n);
        if (listed) {
            rc = list_blocked(finished);
            if (!rc && !list_.empty()) {
                *listed = true;
                return KGX_OK;
            }
        }
        if (!rc)
            rc = inflate(ctx, finished, len);
        *text = text_;
    } else if (joined) {
        joined_.clear();
        joined_.swap(tail_);
        joined_.append(block, n);
        *text = joined_.data();
        *len = joined_.size();
    } else {
        *text = block;
        *len = n;
    }
    if (rc || finished)
        reset();
    return rc;
}

/* the complete members at the front of tail_ into text_ */
int GzipBodyReader::inflate(kgx_ctx *ctx, bool finished, size_t *len)
{
    if (members_ && tail_.size() >= 2 && !((unsigned char)tail_[0] == 0x1f && (unsigned char)tail_[1] == 0x8b))
        tail_.clear(); /* trailing bytes that are no gzip */
    uint64_t members = 0, blocked = 0, out_bytes = 0, consumed = 0, out_len = 0;
    if (int rc = kgx_gunzip_scan(tail_.data(), tail_.size(), finished, &members, &blocked, &out_bytes, &consumed))
        return rc;
    /* blocked members state their sizes; a plain member's is found by trying */
    size_t cap = (size_t)out_bytes + 64;
    if (members > blocked && finished)
        cap += 6 * tail_.size() + (size_t(1) << 20);
    for (;;) {
        if (cap > text_cap_) {
            if (text_)
                kgx_host_free(text_);
            text_ = nullptr;
            text_cap_ = 0;
            void *q = nullptr;
            if (int rc = kgx_host_alloc(cap, &q))
                return rc;
            text_ = static_cast<char *>(q);
            text_cap_ = cap;
        }
        kgx_gunzip_stats gs;
        const int rc = kgx_gunzip(ctx, tail_.data(), tail_.size(), finished, text_, text_cap_, &out_len, &consumed, &gs);
        if (rc == KGX_ERANGE && members > blocked) {
            cap = text_cap_ * 2;
            continue;
        }
        if (rc)
            return rc;
        members_ += gs.members;
        last_members_ = gs.members;
        break;
    }
    tail_.erase(0, (size_t)consumed);
    *len = (size_t)out_len;
    return KGX_OK;
}

}  // namespace kgx
