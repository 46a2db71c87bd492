/*
 * kgx_gzip.h -- gzip framing (RFC 1952), host code, no HIP: member header
 * and trailer, blocked members (BGZF: an extra subfield "BC" of length 2
 * holding BSIZE = the member's total size - 1, so its extent is known
 * without decoding), and one member's decode with both trailer checks
 * (CRC-32 and ISIZE), over kgx_inflate.h.
 */
#pragma once

#include <string>

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
