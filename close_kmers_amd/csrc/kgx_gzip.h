/*
 * kgx_gzip.h -- gzip framing (RFC 1952), host code, no HIP: member header
 * and trailer, blocked members (BGZF: an extra subfield "BC" of length 2
 * holding BSIZE = the member's total size - 1, so its extent is known
 * without decoding), and one member's decode with both trailer checks
 * (CRC-32 and ISIZE), over kgx_inflate.h.
 */
#pragma once

#include <string>
#include <vector>

#include "kgx_inflate.h"

namespace kgx {

/* framing failures; they continue the INF_* numbering in status words and
 * messages */
enum GzipReason : uint32_t {
    GZ_NOT_GZIP = 32,     /* no 1f 8b where a member must start */
    GZ_METHOD = 33,       /* CM != 8 */
    GZ_RESERVED_FLAG = 34, /* FLG bits 5..7 */
    GZ_TRUNCATED = 35,    /* the input ends inside a member and no more will come */
    GZ_BSIZE = 36,        /* BSIZE + 1 does not cover the header and the trailer */
    GZ_BLOCKED_ISIZE = 37, /* a blocked member with ISIZE above 65,536 */
    GZ_HEADER_CRC = 38,   /* FHCRC differs */
};

inline const char *gzip_reason_text(uint32_t r)
{
    switch (r) {
    case GZ_NOT_GZIP: return "not a gzip member";
    case GZ_METHOD: return "compression method is not deflate";
    case GZ_RESERVED_FLAG: return "reserved flag bits set";
    case GZ_TRUNCATED: return "member cut short";
    case GZ_BSIZE: return "BSIZE does not cover the header and trailer";
    case GZ_BLOCKED_ISIZE: return "blocked member with ISIZE above 65536";
    case GZ_HEADER_CRC: return "header CRC mismatch";
    default: return inflate_reason_text(r);
    }
}

inline const uint32_t *crc32_table()
{
    static const struct Table {
        uint32_t t[256];
        Table()
        {
            for (uint32_t i = 0; i < 256; i++)
                t[i] = crc32_table_entry(i);
        }
    } T;
    return T.t;
}

inline uint32_t crc32_of(const uint8_t *p, size_t n)
{
    uint32_t reg = 0xffffffffu;
    const uint32_t *t = crc32_table();
    while (n) {
        const uint32_t k = n > (1u << 30) ? (1u << 30) : (uint32_t)n;
        reg = crc32_run(t, reg, p, k);
        p += k;
        n -= k;
    }
    return ~reg;
}

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline uint32_t le32(const uint8_t *p) { return le16(p) | le16(p + 2) << 16; }

struct GzipHeader {
    uint32_t header_len = 0; /* through FHCRC: the deflate data starts here */
    bool blocked = false;
    uint32_t bsize = 0; /* blocked: the member's total size - 1 */
};

enum { GZ_HDR_OK = 0, GZ_HDR_MORE = 1, GZ_HDR_BAD = 2 };

/* the member header at p[0, n): GZ_HDR_OK, GZ_HDR_MORE (n ends inside it) or
 * GZ_HDR_BAD with *reason */
inline int gzip_header(const uint8_t *p, size_t n, GzipHeader *h, uint32_t *reason)
{
    if (n >= 1 && p[0] != 0x1f) {
        *reason = GZ_NOT_GZIP;
        return GZ_HDR_BAD;
    }
    if (n >= 2 && p[1] != 0x8b) {
        *reason = GZ_NOT_GZIP;
        return GZ_HDR_BAD;
    }
    if (n >= 3 && p[2] != 8) {
        *reason = GZ_METHOD;
        return GZ_HDR_BAD;
    }
    if (n >= 4 && (p[3] & 0xe0)) {
        *reason = GZ_RESERVED_FLAG;
        return GZ_HDR_BAD;
    }
    if (n < 10)
        return GZ_HDR_MORE;
    const uint32_t flg = p[3];
    size_t at = 10;
    *h = GzipHeader{};
    if (flg & 4) { /* FEXTRA */
        if (n < at + 2)
            return GZ_HDR_MORE;
        const size_t xlen = le16(p + at);
        at += 2;
        if (n < at + xlen)
            return GZ_HDR_MORE;
        for (size_t q = at; q + 4 <= at + xlen;) {
            const size_t slen = le16(p + q + 2);
            if (q + 4 + slen > at + xlen)
                break;
            if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) {
                h->blocked = true;
                h->bsize = le16(p + q + 4);
            }
            q += 4 + slen;
        }
        at += xlen;
    }
    for (uint32_t bit : {8u, 16u}) /* FNAME, FCOMMENT: zero-terminated */
        if (flg & bit) {
            while (at < n && p[at])
                at++;
            if (at >= n)
                return GZ_HDR_MORE;
            at++;
        }
    if (flg & 2) { /* FHCRC: the low 16 bits of the header's CRC-32 */
        if (n < at + 2)
            return GZ_HDR_MORE;
        if ((crc32_of(p, at) & 0xffffu) != le16(p + at)) {
            *reason = GZ_HEADER_CRC;
            return GZ_HDR_BAD;
        }
        at += 2;
    }
    h->header_len = (uint32_t)at;
    return GZ_HDR_OK;
}

constexpr uint32_t GZ_BLOCKED_ISIZE_MAX = 65536;

struct GzipBlocked {
    uint64_t total;    /* the member's bytes, header through trailer */
    uint32_t data_len; /* deflate bytes between them */
    uint32_t isize, crc;
};

/* the extent of the blocked member at p[0, n) whose header is h: 0 and *b,
 * 1 = not all of it is there yet, or 2 + the failing reason */
inline int gzip_blocked_extent(const uint8_t *p, uint64_t n, const GzipHeader &h, GzipBlocked *b)
{
    const uint64_t total = (uint64_t)h.bsize + 1;
    if (total < (uint64_t)h.header_len + 8)
        return 2 + GZ_BSIZE;
    if (total > n)
        return 1;
    const uint32_t isize = le32(p + total - 4);
    if (isize > GZ_BLOCKED_ISIZE_MAX)
        return 2 + GZ_BLOCKED_ISIZE;
    *b = GzipBlocked{total, (uint32_t)(total - h.header_len - 8), isize, le32(p + total - 8)};
    return 0;
}

/* one member's deflate data [in, in_end) (a plain member: in_end = the end of
 * the input) into [out, out + cap), then the trailer: the result's reason is
 * INF_OUTPUT_SHORT / INF_CRC when a trailer check fails.  With `blocked`
 * (extent known) the trailer is the 8 bytes at in_end and cap is ISIZE;
 * otherwise it follows the stream's last bit, *member_end is where the member
 * ends, and a trailer past in_end is INF_INPUT_END. */
inline InflateResult gzip_member_inflate(const uint8_t *in, const uint8_t *in_end, bool blocked, uint8_t *out,
                                         size_t cap, InflateTables *t, InflateStats *st, const uint8_t **member_end)
{
    HostIO io;
    InflateResult r = inflate_raw(in, in_end, out, out + cap, t, st, io);
    if (r.reason)
        return r;
    const uint8_t *trailer = blocked ? in_end : in + (r.bit_pos + 7) / 8;
    if (!blocked && in_end - trailer < 8) {
        r.reason = INF_INPUT_END;
        r.bit_pos = (uint64_t)(in_end - in) * 8;
        return r;
    }
    if (member_end)
        *member_end = trailer + 8;
    /* ISIZE is the length modulo 2^32 */
    if (le32(trailer + 4) != (uint32_t)r.out_len)
        r.reason = (uint32_t)r.out_len < le32(trailer + 4) ? INF_OUTPUT_SHORT : INF_OUTPUT_FULL;
    else if (crc32_of(out, r.out_len) != le32(trailer))
        r.reason = INF_CRC;
    r.trailer = r.reason != INF_OK;
    return r;
}

}  // namespace kgx

/* ---- the front end of a body that may be gzip (kgx_gunzip.cpp) ------------ */

struct kgx_ctx;

namespace kgx {

enum GzipBody { GZ_BODY_UNKNOWN, GZ_BODY_HELD, GZ_BODY_TEXT, GZ_BODY_GZIP };

/* The sniff at the start of a body (`fresh`: its parser in the start state
 * with nothing carried), over the bytes held so far followed by the new
 * block: 1f 8b 08 makes the whole body gzip; a start shorter than gzip's
 * fixed header (10 bytes) that may still be one is held until more arrives
 * or the body ends.  Text pays the sniff and nothing else. */
inline GzipBody gzip_sniff(const char *held, size_t n_held, const char *block, size_t n, bool finished, bool fresh)
{
    auto byte = [&](size_t i) { return (unsigned char)(i < n_held ? held[i] : block[i - n_held]); };
    const size_t have = n_held + n;
    if (!fresh || have == 0 || byte(0) != 0x1f)
        return GZ_BODY_TEXT;
    if (have < 3)
        return finished ? GZ_BODY_TEXT : GZ_BODY_HELD;
    if (byte(1) != 0x8b || byte(2) != 8)
        return GZ_BODY_TEXT;
    return have < 10 && !finished ? GZ_BODY_HELD : GZ_BODY_GZIP;
}

/* a complete blocked member of a block: its deflate data at in_off of the
 * block's compressed bytes, its text at out_off of the block's text */
struct GzipListed {
    uint64_t in_off, out_off;
    uint32_t in_len, out_len, crc;
};

/* A body arriving in blocks, as text: the sniff, then either the caller's own
 * bytes (a text body; the held start and the block joined if bytes were
 * held) or the text of the block's complete gzip members, inflated on ctx
 * (kgx_gunzip) into pinned memory (kgx_host_alloc).  A plain (non-blocked)
 * member is held until the body's last block.  Trailing bytes after a member
 * that are no gzip are ignored, as gzip does.  The body ends with its last
 * block or with an error: the next feed() starts one. */
class GzipBodyReader {
public:
    GzipBodyReader() = default;
    GzipBodyReader(const GzipBodyReader &) = delete;
    GzipBodyReader &operator=(const GzipBodyReader &) = delete;
    ~GzipBodyReader();
    /* one block; `fresh` matters only while the body's kind is undecided.
     * KGX_OK with *text = null: the bytes are held, nothing to process yet;
     * else *text, *len (valid until the next call) and gzip() describe them */
    int feed(kgx_ctx *ctx, const char *block, size_t n, bool finished, bool fresh, const char **text, size_t *len);
    /* feed() for a caller that inflates blocked members itself, on the device
     * into a buffer of its own (the fq handler under option "fq_body_device"):
     * when the body is gzip and every complete member of the block is blocked,
     * nothing is inflated -- *listed is set, list() describes the members
     * (in_off into compressed(), out_off counting from 0) and the caller runs
     * them in groups through inflate_listed(), then calls listed_done().  Any
     * other block is feed()'s (a plain member: host text at `finished`). */
    int feed_listed(kgx_ctx *ctx, const char *block, size_t n, bool finished, bool fresh, const char **text,
                    size_t *len, bool *listed);
    const std::vector<GzipListed> &list() const { return list_; }
    const char *compressed() const { return tail_.data(); }
    size_t compressed_len() const { return list_len_; } /* bytes of compressed() the listed members span */
    /* members [first, first + count) of list(), read from d_gz (compressed()
     * uploaded) on ctx's stream; member m's text goes to d_out + out_base +
     * (its out_off - the first one's).  Synchronous.  A bad member is
     * KGX_EFORMAT, named by its number in the block as feed() names it. */
    int inflate_listed(kgx_ctx *ctx, const void *d_gz, uint32_t first, uint32_t count, void *d_out,
                       uint64_t out_base);
    /* the listed members are done with: their bytes leave the reader, and the
     * body ends if the block was its last */
    void listed_done(bool finished);
    /* the block's members again, all on the host (a record too long for the
     * device): the text feed() would have given */
    int inflate_listed_on_host(kgx_ctx *ctx, bool finished, const char **text, size_t *len);
    uint64_t last_members() const { return last_members_; } /* members the last feed() inflated to host text */
    void reset();
    GzipBody body() const { return body_; }
    bool gzip() const { return gzip_; } /* the text of the last feed() was inflated */

private:
    int inflate(kgx_ctx *ctx, bool finished, size_t *len);
    int list_blocked(bool finished);
    std::vector<GzipListed> list_;
    size_t list_len_ = 0;
    uint64_t last_members_ = 0;
    GzipBody body_ = GZ_BODY_UNKNOWN; /* of the body in progress */
    bool gzip_ = false;
    std::string tail_;     /* held first bytes / compressed bytes not consumed yet */
    std::string joined_;   /* held bytes that were text after all, and the block */
    uint64_t members_ = 0; /* members inflated so far in this body */
    char *text_ = nullptr; /* inflated text, pinned */
    size_t text_cap_ = 0;
};

}  // namespace kgx
