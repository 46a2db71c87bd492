/*
 * kgx_inflate.h -- RFC 1951 (DEFLATE) decoding, written once for the host
 * and the device, with no library behind it.
 *
 * inflate_raw() decodes one raw deflate stream from [in, in_end) into
 * [out, out_end) and touches nothing outside the two ranges for any input:
 * every refill of the bit buffer is checked against in_end, every literal and
 * every byte of a match against out_end, and every match distance against the
 * bytes this stream has already produced.  Stored, fixed-Huffman and
 * dynamic-Huffman blocks, any number of blocks.  A malformed stream ends with
 * a reason (INF_*) and the input bit position at which it was seen.
 *
 * The decoder is a template over an IO policy:
 *   HostIO   one thread: bytes are stored one at a time;
 *   WaveIO   (kgx_inflate.hip) one wave: the symbol decode is wave-uniform
 *            (every lane holds the same bit buffer and runs the same
 *            branches), the tables are built and the bytes moved by the lanes
 *            together.
 * The policy gives lane()/lanes() for the cooperative loops, sync() between a
 * table's construction and its use, literal()/match()/stored()/flush() for
 * the bytes, and uni(): a value every lane holds alike, which the device keeps
 * in scalar registers from there on (the input words and table entries come
 * back from memory in vector registers).  Everything else, every bound included, is the same code.
 *
 * Code tables (InflateTables, 3.6 KB; on the device in the wave's own LDS):
 * the canonical code as counts per length and symbols in code order (the walk
 * of RFC 1951 3.2.2 one bit at a time), and in front of it a primary table
 * indexed by the next 10 (literal/length) or 8 (distance) input bits, whose
 * entries are made by running that same walk over the index: one decoder,
 * and the fast table cannot disagree with it.
 *
 * Also here: CRC-32 (the gzip polynomial, reflected) bytewise over a table,
 * and the GF(2) arithmetic that joins the CRC states of adjacent slices.
 */
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define KGX_INF_HD __host__ __device__
#else
#define KGX_INF_HD
#endif

namespace kgx {

enum InflateReason : uint32_t {
    INF_OK = 0,
    INF_BLOCK_TYPE = 1,     /* block type 3 */
    INF_STORED_LEN = 2,     /* stored block: LEN != ~NLEN */
    INF_OVERSUBSCRIBED = 3, /* a code-length set that is over-subscribed */
    INF_INCOMPLETE = 4,     /* an incomplete set that is not one of the single-code cases */
    INF_REPEAT_FIRST = 5,   /* code 16 with no previous length */
    INF_REPEAT_OVERRUN = 6, /* a repeat running past HLIT + HDIST */
    INF_NO_EOB = 7,         /* no code for the end-of-block symbol */
    INF_BAD_SYMBOL = 8,     /* length symbol above 285, distance symbol above 29 */
    INF_TOO_MANY_CODES = 9, /* HLIT above 286 or HDIST above 30 */
    INF_BAD_CODE = 10,      /* input bits that are no code of an incomplete set */
    INF_DISTANCE = 11,      /* a match reaching before the stream's first byte */
    INF_INPUT_END = 12,     /* the input ends inside the stream */
    INF_OUTPUT_FULL = 13,   /* more output than [out, out_end) holds */
    INF_OUTPUT_SHORT = 14,  /* gzip: fewer bytes than ISIZE */
    INF_CRC = 15,           /* gzip: CRC-32 of the output differs from the trailer's */
    INF_REASONS = 16
};

inline const char *inflate_reason_text(uint32_t r)
{
    static const char *const T[INF_REASONS] = {
        "ok", "block type 3", "stored block LEN/NLEN mismatch", "over-subscribed code lengths",
        "incomplete code lengths", "length repeat with no previous length", "length repeat past HLIT + HDIST",
        "no end-of-block code", "length or distance symbol out of range", "too many length or distance codes",
        "invalid code", "distance before the start of the member", "input ends inside the stream",
        "output longer than ISIZE", "output shorter than ISIZE", "CRC-32 mismatch"};
    return r < INF_REASONS ? T[r] : "unknown";
}

/* what a stream exercised; tests use it to show a fixture hits its target */
struct InflateStats {
    uint32_t stored_blocks, fixed_blocks, dynamic_blocks;
    uint32_t max_code_len; /* longest code length of any dynamic block's literal/length or distance set */
    uint32_t max_distance;
    uint32_t max_length;
    uint32_t overlap; /* 1: some match had distance < length */
    uint32_t matches;
};

struct InflateResult {
    uint32_t reason;
    uint32_t trailer; /* gzip: 1 when the reason is a trailer check's (ISIZE, CRC-32), not the stream's */
    uint64_t out_len; /* bytes produced (also on failure: those before it) */
    uint64_t bit_pos; /* input bits consumed; on failure, where it was seen */
};

enum { INF_FAST_L = 10, INF_FAST_D = 8, INF_MAX_L = 288, INF_MAX_D = 32 };

struct InflateTables {
    uint16_t fast_l[1 << INF_FAST_L]; /* (symbol << 4) | length, 0 = a longer code */
    uint16_t fast_d[1 << INF_FAST_D];
    uint16_t sym_l[INF_MAX_L], sym_d[INF_MAX_D]; /* symbols in code order */
    uint16_t cnt_l[16], cnt_d[16];               /* codes per length */
    uint16_t offs[16];
    uint8_t lens[INF_MAX_L + INF_MAX_D];
};

/* ---- CRC-32 -------------------------------------------------------------- */

constexpr uint32_t CRC32_POLY = 0xedb88320u;

KGX_INF_HD inline uint32_t crc32_table_entry(uint32_t i)
{
    uint32_t c = i;
    for (int k = 0; k < 8; k++)
        c = (c & 1u) ? (c >> 1) ^ CRC32_POLY : c >> 1;
    return c;
}

/* the register after `n` more bytes; the register starts at 0xffffffff and
 * the CRC is its complement */
KGX_INF_HD inline uint32_t crc32_run(const uint32_t *table, uint32_t reg, const uint8_t *p, uint32_t n)
{
    for (uint32_t i = 0; i < n; i++)
        reg = table[(reg ^ p[i]) & 0xffu] ^ (reg >> 8);
    return reg;
}

/* a * b mod the CRC polynomial; bit 31 is x^0 (reflected) */
KGX_INF_HD inline uint32_t crc32_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m)
            p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC32_POLY : b >> 1;
    }
    return p;
}

/* x^(8 n) mod the CRC polynomial.  The register is linear in its start value:
 * running n bytes from register r gives mulmod(r, x^(8n)) ^ (the run from 0),
 * so slices run separately (the first from 0xffffffff, the others from 0)
 * join as the XOR of each slice's register times x^(8 * bytes after it). */
KGX_INF_HD inline uint32_t crc32_xpow8(uint32_t n)
{
    uint32_t r = 1u << 31, sq = 1u << 23; /* 1, x^8 */
    for (; n; n >>= 1) {
        if (n & 1u)
            r = crc32_mulmod(r, sq);
        sq = crc32_mulmod(sq, sq);
    }
    return r;
}

/* ---- the IO policy of one host thread ------------------------------------ */

struct HostIO {
    KGX_INF_HD uint32_t lane() const { return 0; }
    KGX_INF_HD uint32_t lanes() const { return 1; }
    KGX_INF_HD void sync() const {}
    KGX_INF_HD uint32_t uni(uint32_t v) const { return v; }
    KGX_INF_HD uint64_t uni(uint64_t v) const { return v; }
    KGX_INF_HD void literal(uint8_t *dst, uint8_t v) { *dst = v; }
    KGX_INF_HD void flush() {}
    /* dist <= bytes before dst, dst + len <= out_end: checked by the caller */
    KGX_INF_HD void match(uint8_t *dst, uint32_t dist, uint32_t len)
    {
        const uint8_t *src = dst - dist;
        for (uint32_t i = 0; i < len; i++)
            dst[i] = src[i];
    }
    KGX_INF_HD void stored(uint8_t *dst, const uint8_t *src, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++)
            dst[i] = src[i];
    }
};

/* ---- the decoder ----------------------------------------------------------- */

namespace inflate_detail {

struct Bits {
    const uint8_t *in0, *in, *end;
    uint64_t buf;
    uint32_t n; /* valid bits in buf */
    template <class IO> KGX_INF_HD void refill(IO &io)
    {
        if (end - in >= 8) {
            uint64_t v;
            memcpy(&v, in, 8);
            buf |= io.uni(v) << n;
            in += (63u - n) >> 3;
            n |= 56u;
        } else {
            while (n <= 56u && in < end) {
                buf |= (uint64_t)io.uni((uint32_t)*in++) << n;
                n += 8;
            }
        }
    }
    KGX_INF_HD void drop(uint32_t k)
    {
        buf >>= k;
        n -= k;
    }
    KGX_INF_HD uint64_t pos() const { return (uint64_t)(in - in0) * 8u - n; }
};

/* the canonical walk over the low bits of `bits`, at most `avail` of them and
 * at most `maxlen` long: the symbol and its length, or length 0 */
template <class IO>
KGX_INF_HD inline uint32_t walk(IO &io, const uint16_t *cnt, const uint16_t *sym, uint32_t bits, uint32_t maxlen,
                                uint32_t *len_out)
{
    int32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= maxlen; len++) {
        code |= (int32_t)(bits & 1u);
        bits >>= 1;
        const int32_t count = (int32_t)io.uni((uint32_t)cnt[len]);
        if (code - count < first) {
            *len_out = len;
            return io.uni((uint32_t)sym[index + (code - first)]);
        }
        index += count;
        first += count;
        first <<= 1;
        code <<= 1;
    }
    *len_out = 0;
    return 0;
}

/* counts, symbols in code order and the primary table of one code from
 * lens[0, n).  0, INF_OVERSUBSCRIBED or INF_INCOMPLETE; *max_len = the longest
 * length. */
template <class IO>
KGX_INF_HD inline uint32_t build(IO &io, const uint8_t *lens, uint32_t n, uint16_t *cnt, uint16_t *sym, uint16_t *offs,
                             uint16_t *fast, uint32_t fast_bits, bool strict, uint32_t *max_len)
{
    /* the counts and the order are a few hundred wave-uniform steps; every
     * lane stores the same values */
    for (uint32_t l = 0; l < 16; l++)
        cnt[l] = 0;
    io.sync();
    for (uint32_t s = 0; s < n; s++)
        cnt[lens[s]]++;
    io.sync();
    uint32_t longest = 0;
    int32_t left = 1;
    for (uint32_t l = 1; l < 16; l++) {
        left <<= 1;
        left -= (int32_t)cnt[l];
        if (left < 0)
            return INF_OVERSUBSCRIBED;
        if (cnt[l])
            longest = l;
    }
    *max_len = longest;
    offs[1] = 0;
    for (uint32_t l = 1; l < 15; l++)
        offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    io.sync();
    for (uint32_t s = 0; s < n; s++)
        if (lens[s])
            sym[offs[lens[s]]++] = (uint16_t)s;
    io.sync();
    /* the primary table: the lanes share the indexes, so here the walk's
     * values differ from lane to lane (no uni()) */
    HostIO each;
    for (uint32_t i = io.lane(); i < (1u << fast_bits); i += io.lanes()) {
        uint32_t len;
        const uint32_t s = walk(each, cnt, sym, i, fast_bits, &len);
        fast[i] = (uint16_t)(len ? (s << 4) | len : 0u);
    }
    io.sync();
    /* incomplete: never for the code-length code (strict); otherwise allowed
     * with no code at all (a block without matches has no distance code) and
     * with a single code of length 1 */
    if (left > 0 && (strict || !(cnt[0] == n || (longest == 1 && cnt[1] == 1))))
        return INF_INCOMPLETE;
    return INF_OK;
}

/* the next symbol of a code: its value, or INF_ERR + reason */
constexpr uint32_t INF_ERR = 1u << 16;
template <class IO>
KGX_INF_HD inline uint32_t decode(IO &io, Bits &b, const uint16_t *cnt, const uint16_t *sym, const uint16_t *fast,
                              uint32_t fast_bits)
{
    if (b.n < 15u)
        b.refill(io);
    const uint32_t e = io.uni((uint32_t)fast[b.buf & ((1u << fast_bits) - 1u)]);
    if (e) {
        const uint32_t len = e & 15u;
        if (len > b.n)
            return INF_ERR + INF_INPUT_END;
        b.drop(len);
        return e >> 4;
    }
    uint32_t len;
    const uint32_t s = walk(io, cnt, sym, (uint32_t)b.buf, b.n < 15u ? b.n : 15u, &len);
    if (!len)
        return INF_ERR + (b.n < 15u ? (uint32_t)INF_INPUT_END : (uint32_t)INF_BAD_CODE);
    b.drop(len);
    return s;
}

}  // namespace inflate_detail

template <class IO>
KGX_INF_HD inline InflateResult inflate_raw(const uint8_t *in, const uint8_t *in_end, uint8_t *out, uint8_t *out_end,
                                        InflateTables *t, InflateStats *st, IO &io)
{
    using namespace inflate_detail;
    static const uint16_t LBASE[29] = {3,  4,  5,  6,  7,  8,  9,  10, 11,  13,  15,  17,  19,  23, 27,
                                       31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t LEXT[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t DBASE[30] = {1,   2,   3,   4,   5,   7,    9,    13,   17,   25,   33,   49,   65,    97,    129,
                                       193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t DEXT[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t ORDER[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

    Bits b{in, in, in_end, 0, 0};
    uint8_t *o = out;
    InflateStats s{};
    uint32_t reason = INF_OK;
    uint64_t at = 0; /* the bit position of a failure */
#define INF_FAIL(r)       \
    do {                  \
        reason = (r);     \
        at = b.pos();     \
        goto done;        \
    } while (0)
#define INF_NEED(k)                 \
    do {                            \
        if (b.n < (uint32_t)(k)) {  \
            b.refill(io);           \
            if (b.n < (uint32_t)(k)) \
                INF_FAIL(INF_INPUT_END); \
        }                           \
    } while (0)

    for (uint32_t last = 0; !last;) {
        INF_NEED(3);
        last = (uint32_t)b.buf & 1u;
        const uint32_t type = ((uint32_t)b.buf >> 1) & 3u;
        if (type == 3)
            INF_FAIL(INF_BLOCK_TYPE);
        b.drop(3);
        if (type == 0) {
            s.stored_blocks++;
            b.drop(b.n & 7u);
            INF_NEED(32);
            const uint32_t len = (uint32_t)b.buf & 0xffffu, nlen = ((uint32_t)(b.buf >> 16)) & 0xffffu;
            if (len != (nlen ^ 0xffffu))
                INF_FAIL(INF_STORED_LEN);
            b.drop(32);
            /* whole bytes still in the bit buffer go back to the input */
            b.in -= b.n >> 3;
            b.n = 0;
            b.buf = 0;
            if ((size_t)(b.end - b.in) < len) {
                b.in = b.end;
                INF_FAIL(INF_INPUT_END);
            }
            if ((size_t)(out_end - o) < len)
                INF_FAIL(INF_OUTPUT_FULL);
            io.flush();
            io.stored(o, b.in, len);
            b.in += len;
            o += len;
            continue;
        }
        uint32_t nl, nd;
        if (type == 1) {
            s.fixed_blocks++;
            nl = 288;
            nd = 32; /* complete codes; 286, 287 and 30, 31 never valid in the data */
            for (uint32_t i = io.lane(); i < 288u + 32u; i += io.lanes())
                t->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
            io.sync();
        } else {
            s.dynamic_blocks++;
            INF_NEED(14);
            nl = ((uint32_t)b.buf & 31u) + 257u;
            nd = (((uint32_t)b.buf >> 5) & 31u) + 1u;
            const uint32_t nc = (((uint32_t)b.buf >> 10) & 15u) + 4u;
            if (nl > 286u || nd > 30u)
                INF_FAIL(INF_TOO_MANY_CODES);
            b.drop(14);
            /* the code-length code: its 19 lengths, and its tables in the
             * distance code's place */
            for (uint32_t i = io.lane(); i < 19u; i += io.lanes())
                t->lens[i] = 0;
            io.sync();
            for (uint32_t i = 0; i < nc; i++) {
                INF_NEED(3);
                t->lens[ORDER[i]] = (uint8_t)(b.buf & 7u);
                b.drop(3);
            }
            io.sync();
            uint32_t ml;
            uint32_t r = build(io, t->lens, 19, t->cnt_d, t->sym_d, t->offs, t->fast_d, INF_FAST_D, true, &ml);
            if (r)
                INF_FAIL(r);
            uint32_t idx = 0, prev = 0;
            while (idx < nl + nd) {
                const uint32_t sy = decode(io, b, t->cnt_d, t->sym_d, t->fast_d, INF_FAST_D);
                if (sy >= INF_ERR)
                    INF_FAIL(sy - INF_ERR);
                if (sy < 16) {
                    t->lens[idx++] = (uint8_t)sy;
                    prev = sy;
                    continue;
                }
                uint32_t rep, v = 0;
                if (sy == 16) {
                    if (idx == 0)
                        INF_FAIL(INF_REPEAT_FIRST);
                    v = prev;
                    INF_NEED(2);
                    rep = 3u + ((uint32_t)b.buf & 3u);
                    b.drop(2);
                } else if (sy == 17) {
                    INF_NEED(3);
                    rep = 3u + ((uint32_t)b.buf & 7u);
                    b.drop(3);
                } else {
                    INF_NEED(7);
                    rep = 11u + ((uint32_t)b.buf & 127u);
                    b.drop(7);
                }
                if (idx + rep > nl + nd)
                    INF_FAIL(INF_REPEAT_OVERRUN);
                for (uint32_t k = 0; k < rep; k++)
                    t->lens[idx + k] = (uint8_t)v;
                idx += rep;
                prev = v;
            }
            io.sync();
            if (t->lens[256] == 0)
                INF_FAIL(INF_NO_EOB);
        }
        {
            uint32_t ml, md;
            uint32_t r = build(io, t->lens, nl, t->cnt_l, t->sym_l, t->offs, t->fast_l, INF_FAST_L, false, &ml);
            if (r)
                INF_FAIL(r);
            r = build(io, t->lens + nl, nd, t->cnt_d, t->sym_d, t->offs, t->fast_d, INF_FAST_D, false, &md);
            if (r)
                INF_FAIL(r);
            if (type == 2) {
                if (ml > s.max_code_len)
                    s.max_code_len = ml;
                if (md > s.max_code_len)
                    s.max_code_len = md;
            }
        }
        for (;;) {
            uint32_t sy = decode(io, b, t->cnt_l, t->sym_l, t->fast_l, INF_FAST_L);
            if (sy < 256) {
                if (o == out_end)
                    INF_FAIL(INF_OUTPUT_FULL);
                io.literal(o, (uint8_t)sy);
                o++;
                continue;
            }
            if (sy == 256)
                break;
            if (sy >= INF_ERR)
                INF_FAIL(sy - INF_ERR);
            sy -= 257;
            if (sy >= 29)
                INF_FAIL(INF_BAD_SYMBOL);
            INF_NEED(LEXT[sy]);
            const uint32_t len = LBASE[sy] + ((uint32_t)b.buf & ((1u << LEXT[sy]) - 1u));
            b.drop(LEXT[sy]);
            const uint32_t ds = decode(io, b, t->cnt_d, t->sym_d, t->fast_d, INF_FAST_D);
            if (ds >= INF_ERR)
                INF_FAIL(ds - INF_ERR);
            if (ds >= 30)
                INF_FAIL(INF_BAD_SYMBOL);
            INF_NEED(DEXT[ds]);
            const uint32_t dist = DBASE[ds] + ((uint32_t)b.buf & ((1u << DEXT[ds]) - 1u));
            b.drop(DEXT[ds]);
            if (dist > (size_t)(o - out))
                INF_FAIL(INF_DISTANCE);
            if (len > (size_t)(out_end - o))
                INF_FAIL(INF_OUTPUT_FULL);
            io.match(o, dist, len);
            o += len;
            s.matches++;
            if (dist > s.max_distance)
                s.max_distance = dist;
            if (len > s.max_length)
                s.max_length = len;
            if (dist < len)
                s.overlap = 1;
        }
    }
    at = b.pos();
done:
#undef INF_FAIL
#undef INF_NEED
    io.flush();
    *st = s;
    return InflateResult{reason, 0u, (uint64_t)(o - out), at};
}

}  // namespace kgx
