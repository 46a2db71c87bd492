/*
 * kgx_fq_parse.hip -- the FASTQ parser on the device (include/kgx.h
 * kgx_fq_parse*): text in device memory -> bases,
 * read_offsets, ids, id_offsets in the buffers kgx_fq_proteins reads.
 *
 * The parser is FastqParser::parse_char (fastq_parser.h:40-150): seven states
 * (start, id, defline, data, plus start, plus line, quality) over six byte
 * classes ('\n', '@', '+', blank, ASCII letter, other).  What a byte does
 * depends on the state before it, so a run of bytes is a map from entry state
 * to exit state: 7 x 3 bits in one word, and maps compose associatively.
 *
 *   map    a lane builds the map of its 16 bytes, the wave composes by
 *          shuffles, the workgroup through LDS: one map per 4096-byte tile
 *   state  one workgroup scans the tile maps: the entry state of every tile
 *   count  with the entry state known, per lane its entry state (kept, one
 *          byte), per tile the id bytes, base bytes, record ends and newlines,
 *          and the first offending byte (one atomicMin per tile that has one)
 *   sums   one workgroup: the exclusive sums of the tiles' counts, the totals
 *   write  id bytes and base bytes compacted through LDS to their places; the
 *          lane that sees record end k writes read_offsets[k + 1] and
 *          id_offsets[k + 1]
 *   no_id  the reads without an id, counted
 *
 * Separate launches: no kernel waits on another workgroup.  Strict mode is the
 * lenient machine cut at the first offending byte e: the host reads e with the
 * totals and, when there is one, runs count and sums again over [0, e) (once
 * per file: the error ends its parse).  The tiles' entry states do not depend
 * on what follows them.
 */
#include "kgx_device.h"
#include "kgx_rt.h"

using namespace kgx;

namespace {

constexpr uint32_t SPAN = 4096;      /* bytes per workgroup: 256 lanes x 16 */
constexpr uint32_t LANE_BYTES = 16;
constexpr uint32_t WG = 256, WAVES = 4;

enum : uint32_t { S_START, S_ID, S_DEF, S_DATA, S_PLUS_START, S_PLUS, S_QUAL, N_STATES };
enum : uint32_t { C_NL, C_AT, C_PLUS, C_BLANK, C_LETTER, C_OTHER, N_CLASSES };
enum : uint32_t { EV_ID = 1, EV_BASE = 2, EV_END = 4, EV_BAD = 8 };

constexpr uint32_t next_state(uint32_t s, uint32_t c)
{
    switch (s) {
    case S_START: return c == C_AT ? S_ID : S_START;
    case S_ID: return c == C_NL ? S_DATA : c == C_BLANK ? S_DEF : S_ID;
    case S_DEF: return c == C_NL ? S_DATA : S_DEF;
    case S_DATA: return c == C_NL ? S_PLUS_START : S_DATA;
    case S_PLUS_START: return c == C_PLUS ? S_PLUS : S_PLUS_START;
    case S_PLUS: return c == C_NL ? S_QUAL : S_PLUS;
    default: return c == C_NL ? S_START : S_QUAL;
    }
}

constexpr uint32_t event_of(uint32_t s, uint32_t c)
{
    switch (s) {
    case S_START: return c == C_AT ? 0 : EV_BAD;
    case S_ID: return (c == C_NL || c == C_BLANK) ? 0 : EV_ID;
    case S_DATA: return c == C_NL ? 0 : c == C_LETTER ? EV_BASE : EV_BAD;
    case S_PLUS_START: return c == C_PLUS ? 0 : EV_BAD;
    case S_QUAL: return c == C_NL ? EV_END : 0;
    default: return 0;
    }
}

/* class c as a map: state s -> bits [3s, 3s + 3) */
constexpr uint32_t map_word(uint32_t c)
{
    uint32_t w = 0;
    for (uint32_t s = 0; s < N_STATES; s++)
        w |= next_state(s, c) << (3 * s);
    return w;
}

/* class c's events: state s -> bits [4s, 4s + 4) */
constexpr uint32_t event_word(uint32_t c)
{
    uint32_t w = 0;
    for (uint32_t s = 0; s < N_STATES; s++)
        w |= event_of(s, c) << (4 * s);
    return w;
}

constexpr uint32_t IDENTITY = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12 | 5u << 15 | 6u << 18;
constexpr uint32_t NL_BIT = 1u << 31; /* in a byte's map word: the byte is '\n' */
constexpr uint64_t NO_ERROR = ~0ull;  /* the error key: pos << 16 | code << 8 | byte */

/* the sums a call leaves for the host, uint64 each */
enum : uint32_t {
    SUM_IDS, SUM_BASES, SUM_RECORDS, SUM_NEWLINES, SUM_ERROR, /* after the sums kernel */
    SUM_CONSUMED = 8, SUM_CONSUMED_NL, SUM_IDS_AT_END, SUM_BASES_AT_END, SUM_ERROR_NL, SUM_NO_ID, /* after write */
    SUM_ERROR_KEY = 15, /* the count kernel's atomicMin */
    SUM_WORDS
};

struct ByteWords {
    uint32_t map, events;
};

/* the byte's map and event words: tab[b], filled by the workgroup's 256 lanes */
__device__ __forceinline__ void fill_table(ByteWords *tab, uint32_t tid)
{
    const bool letter = ((tid | 0x20u) - 'a') < 26u;
    const uint32_t c = tid == '\n' ? C_NL
                       : tid == '@' ? C_AT
                       : tid == '+' ? C_PLUS
                       : (tid == ' ' || tid == '\t') ? C_BLANK
                       : letter ? C_LETTER
                                : C_OTHER;
    uint32_t m = map_word(C_OTHER), e = event_word(C_OTHER);
    if (c == C_NL) { m = map_word(C_NL) | NL_BIT; e = event_word(C_NL); }
    if (c == C_AT) { m = map_word(C_AT); e = event_word(C_AT); }
    if (c == C_PLUS) { m = map_word(C_PLUS); e = event_word(C_PLUS); }
    if (c == C_BLANK) { m = map_word(C_BLANK); e = event_word(C_BLANK); }
    if (c == C_LETTER) { m = map_word(C_LETTER); e = event_word(C_LETTER); }
    tab[tid].map = m;
    tab[tid].events = e;
}

/* f, then g: (g o f)(s) for every s */
__device__ __forceinline__ uint32_t then(uint32_t f, uint32_t g)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < N_STATES; s++)
        r |= ((g >> (3u * ((f >> (3u * s)) & 7u))) & 7u) << (3u * s);
    return r;
}

__device__ __forceinline__ uint32_t apply(uint32_t map, uint32_t s) { return (map >> (3u * s)) & 7u; }

/* the lane's bytes text[pos, pos + 16) below n: whole as one uint4 (text is
 * 16-byte aligned and pos a multiple of 16), the text's last ones singly */
__device__ __forceinline__ uint32_t load_lane(const uint8_t *text, uint64_t n, uint64_t pos, uint32_t (&w)[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
    if (pos + LANE_BYTES <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(text + pos);
        w[0] = v.x;
        w[1] = v.y;
        w[2] = v.z;
        w[3] = v.w;
        return LANE_BYTES;
    }
    if (pos >= n)
        return 0;
    const uint32_t valid = (uint32_t)(n - pos);
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++)
        if (j < valid)
            w[j >> 2] |= (uint32_t)text[pos + j] << (8u * (j & 3u));
    return valid;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], uint32_t j) { return (w[j >> 2] >> (8u * (j & 3u))) & 255u; }

/* the map of the lane's bytes */
__device__ __forceinline__ uint32_t lane_map(const ByteWords *tab, const uint32_t (&w)[4], uint32_t valid)
{
    uint32_t m = IDENTITY;
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++)
        if (j < valid)
            m = then(m, tab[byte_of(w, j)].map);
    return m;
}

/* inclusive composition over the wave's lanes, lane 0 first */
__device__ __forceinline__ uint32_t wave_scan_maps(uint32_t m, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(m, d, 64);
        if (lane >= d)
            m = then(o, m);
    }
    return m;
}

template <class T> __device__ __forceinline__ T wave_scan_add(T v, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= d)
            v += o;
    }
    return v;
}

/* 1. a tile's map */
__global__ __launch_bounds__(256) void fq_parse_map_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                           uint32_t *__restrict__ tile_map)
{
    __shared__ ByteWords tab[256];
    __shared__ uint32_t wave_map[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table(tab, tid);
    __syncthreads();
    uint32_t w[4];
    const uint32_t valid = load_lane(text, n, (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES, w);
    const uint32_t inc = wave_scan_maps(lane_map(tab, w, valid), lane);
    if (lane == 63)
        wave_map[wv] = inc;
    __syncthreads();
    if (tid == 0)
        tile_map[blockIdx.x] = then(then(then(wave_map[0], wave_map[1]), wave_map[2]), wave_map[3]);
}

/* 2. one workgroup: every tile's entry state, and the text's end state in
 * tile_state[n_tiles] */
__global__ __launch_bounds__(256) void fq_parse_state_kernel(const uint32_t *__restrict__ tile_map, uint32_t n_tiles,
                                                             uint8_t *__restrict__ tile_state)
{
    __shared__ uint32_t wave_map[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = S_START;
    for (uint32_t base = 0; base < n_tiles; base += WG) {
        const uint32_t i = base + tid;
        const uint32_t inc = wave_scan_maps(i < n_tiles ? tile_map[i] : IDENTITY, lane);
        if (lane == 63)
            wave_map[wv] = inc;
        __syncthreads();
        uint32_t exc = __shfl_up(inc, 1, 64);
        if (lane == 0)
            exc = IDENTITY;
        uint32_t s = carry;
        for (uint32_t k = 0; k < wv; k++)
            s = apply(wave_map[k], s);
        if (i < n_tiles)
            tile_state[i] = (uint8_t)apply(exc, s);
        for (uint32_t k = 0; k < WAVES; k++)
            carry = apply(wave_map[k], carry);
        __syncthreads();
    }
    if (tid == 0)
        tile_state[n_tiles] = (uint8_t)carry;
}

/* the lane's entry state: the tile's, through the earlier waves and lanes */
__device__ __forceinline__ uint32_t lane_entry_state(uint32_t m, uint32_t tile_entry, uint32_t *wave_map, uint32_t lane,
                                                     uint32_t wv)
{
    const uint32_t inc = wave_scan_maps(m, lane);
    if (lane == 63)
        wave_map[wv] = inc;
    __syncthreads();
    uint32_t exc = __shfl_up(inc, 1, 64);
    if (lane == 0)
        exc = IDENTITY;
    uint32_t s = tile_entry;
    for (uint32_t k = 0; k < wv; k++)
        s = apply(wave_map[k], s);
    return apply(exc, s);
}

/* id bytes | base bytes << 16 | record ends << 32 | newlines << 48: a tile has
 * 4096 bytes, so no field carries into the next */
__device__ __forceinline__ uint64_t pack_counts(uint32_t ids, uint32_t bases, uint32_t ends, uint32_t nls)
{
    return (uint64_t)ids | (uint64_t)bases << 16 | (uint64_t)ends << 32 | (uint64_t)nls << 48;
}

/* 3. the lanes' entry states, the tile's counts, the first offending byte */
__global__ __launch_bounds__(256) void fq_parse_count_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                             const uint8_t *__restrict__ tile_state,
                                                             uint8_t *__restrict__ lane_state,
                                                             uint4 *__restrict__ tile_cnt, uint64_t *error_key)
{
    __shared__ ByteWords tab[256];
    __shared__ uint32_t wave_map[WAVES];
    __shared__ uint64_t wave_cnt[WAVES];
    __shared__ unsigned long long tile_key;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table(tab, tid);
    if (tid == 0)
        tile_key = NO_ERROR;
    __syncthreads();
    uint32_t w[4];
    const uint64_t pos = (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES;
    const uint32_t valid = load_lane(text, n, pos, w);
    uint32_t s = lane_entry_state(lane_map(tab, w, valid), tile_state[blockIdx.x], wave_map, lane, wv);
    lane_state[(uint64_t)blockIdx.x * WG + tid] = (uint8_t)s;
    uint32_t ids = 0, bases = 0, ends = 0, nls = 0;
    uint64_t key = NO_ERROR;
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++) {
        if (j < valid) {
            const uint32_t b = byte_of(w, j);
            const ByteWords t = tab[b];
            const uint32_t ev = (t.events >> (4u * s)) & 15u;
            ids += ev & 1u;
            bases += (ev >> 1) & 1u;
            ends += (ev >> 2) & 1u;
            nls += t.map >> 31;
            if ((ev & EV_BAD) && key == NO_ERROR) {
                const uint32_t code = s == S_START ? (b == '>' ? 1u : 2u) : s == S_DATA ? 3u : 4u;
                key = (pos + j) << 16 | (uint64_t)code << 8 | b;
            }
            s = apply(t.map, s);
        }
    }
    if (key != NO_ERROR)
        atomicMin(&tile_key, (unsigned long long)key);
    uint64_t c = pack_counts(ids, bases, ends, nls);
#pragma unroll
    for (uint32_t d = 32; d; d >>= 1)
        c += __shfl_down(c, d, 64);
    if (lane == 0)
        wave_cnt[wv] = c;
    __syncthreads();
    if (tid == 0) {
        const uint64_t t = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
        tile_cnt[blockIdx.x] = make_uint4((uint32_t)(t & 0xffffu), (uint32_t)(t >> 16 & 0xffffu),
                                          (uint32_t)(t >> 32 & 0xffffu), (uint32_t)(t >> 48));
        if (tile_key != NO_ERROR)
            atomicMin(reinterpret_cast<unsigned long long *>(error_key), tile_key);
    }
}

/* 4. one workgroup: the exclusive sums of the tiles' counts (x ids, y bases,
 * z record ends, w newlines; n <= KGX_FQ_PARSE_MAX keeps them in 32 bits) and
 * the call's sums */
__global__ __launch_bounds__(256) void fq_parse_sums_kernel(const uint4 *__restrict__ tile_cnt, uint32_t n_tiles,
                                                            uint4 *__restrict__ tile_pre, uint64_t *sums)
{
    __shared__ uint4 wave_sum[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint4 carry = make_uint4(0, 0, 0, 0);
    for (uint32_t base = 0; base < n_tiles; base += WG) {
        const uint32_t i = base + tid;
        const uint4 v = i < n_tiles ? tile_cnt[i] : make_uint4(0, 0, 0, 0);
        uint4 inc;
        inc.x = wave_scan_add(v.x, lane);
        inc.y = wave_scan_add(v.y, lane);
        inc.z = wave_scan_add(v.z, lane);
        inc.w = wave_scan_add(v.w, lane);
        if (lane == 63)
            wave_sum[wv] = inc;
        __syncthreads();
        uint4 p = carry;
        for (uint32_t k = 0; k < WAVES; k++) {
            const uint4 ws = wave_sum[k];
            if (k < wv) {
                p.x += ws.x;
                p.y += ws.y;
                p.z += ws.z;
                p.w += ws.w;
            }
            carry.x += ws.x;
            carry.y += ws.y;
            carry.z += ws.z;
            carry.w += ws.w;
        }
        if (i < n_tiles)
            tile_pre[i] = make_uint4(p.x + inc.x - v.x, p.y + inc.y - v.y, p.z + inc.z - v.z, p.w + inc.w - v.w);
        __syncthreads();
    }
    if (tid == 0) {
        sums[SUM_IDS] = carry.x;
        sums[SUM_BASES] = carry.y;
        sums[SUM_RECORDS] = carry.z;
        sums[SUM_NEWLINES] = carry.w;
        sums[SUM_ERROR] = sums[SUM_ERROR_KEY];
    }
    if (tid >= SUM_CONSUMED && tid <= SUM_NO_ID)
        sums[tid] = 0;
}

/* 5. the outputs.  grid = max(1, tiles of [0, n)); n_records, n_ids and
 * n_bases are the sums over [0, n).  read_offsets and id_offsets hold
 * n_records + 2 entries: [0] = 0, one per record end, and the record in
 * progress at n closed by the totals (the host decides whether it is a read).
 * error_pos: the byte whose newline count the host wants (NO_ERROR: none) */
__global__ __launch_bounds__(256) void fq_parse_write_kernel(
    const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ lane_state,
    const uint4 *__restrict__ tile_pre, uint32_t n_records, uint64_t n_ids, uint64_t n_bases, uint64_t error_pos,
    uint8_t *__restrict__ bases, uint64_t *__restrict__ read_offsets, uint8_t *__restrict__ ids,
    uint64_t *__restrict__ id_offsets, uint64_t *sums)
{
    __shared__ ByteWords tab[256];
    __shared__ uint64_t wave_cnt[WAVES];
    __shared__ uint8_t tile_ids[SPAN], tile_bases[SPAN];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table(tab, tid);
    if (blockIdx.x == 0 && tid == 0) {
        read_offsets[0] = 0;
        id_offsets[0] = 0;
        read_offsets[(uint64_t)n_records + 1] = n_bases;
        id_offsets[(uint64_t)n_records + 1] = n_ids;
    }
    __syncthreads();
    uint32_t w[4];
    const uint64_t pos = (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES;
    const uint32_t valid = load_lane(text, n, pos, w);
    const uint32_t s0 = valid ? lane_state[(uint64_t)blockIdx.x * WG + tid] : S_START;
    uint32_t s = s0, ni = 0, nb = 0, ne = 0, nn = 0;
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++) {
        if (j < valid) {
            const ByteWords t = tab[byte_of(w, j)];
            const uint32_t ev = (t.events >> (4u * s)) & 15u;
            ni += ev & 1u;
            nb += (ev >> 1) & 1u;
            ne += (ev >> 2) & 1u;
            nn += t.map >> 31;
            s = apply(t.map, s);
        }
    }
    const uint64_t mine = pack_counts(ni, nb, ne, nn);
    const uint64_t inc = wave_scan_add(mine, lane);
    if (lane == 63)
        wave_cnt[wv] = inc;
    __syncthreads();
    uint64_t before = inc - mine, total = 0;
    for (uint32_t k = 0; k < WAVES; k++) {
        if (k < wv)
            before += wave_cnt[k];
        total += wave_cnt[k];
    }
    const uint4 pre = n ? tile_pre[blockIdx.x] : make_uint4(0, 0, 0, 0);
    uint32_t li = (uint32_t)(before & 0xffffu), lb = (uint32_t)(before >> 16 & 0xffffu);
    uint32_t le = (uint32_t)(before >> 32 & 0xffffu), ln = (uint32_t)(before >> 48);
    s = s0;
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++) {
        if (j < valid) {
            const uint32_t b = byte_of(w, j);
            const ByteWords t = tab[b];
            const uint32_t ev = (t.events >> (4u * s)) & 15u;
            if (ev & EV_ID)
                tile_ids[li++] = (uint8_t)b;
            if (ev & EV_BASE)
                tile_bases[lb++] = (uint8_t)b;
            ln += t.map >> 31;
            if (ev & EV_END) {
                const uint64_t k = (uint64_t)pre.z + le++;
                read_offsets[k + 1] = (uint64_t)pre.y + lb;
                id_offsets[k + 1] = (uint64_t)pre.x + li;
                if (k + 1 == n_records) { /* the last record's end: what the caller has consumed */
                    sums[SUM_CONSUMED] = pos + j + 1;
                    sums[SUM_CONSUMED_NL] = (uint64_t)pre.w + ln;
                    sums[SUM_IDS_AT_END] = (uint64_t)pre.x + li;
                    sums[SUM_BASES_AT_END] = (uint64_t)pre.y + lb;
                }
            }
            if (pos + j == error_pos)
                sums[SUM_ERROR_NL] = (uint64_t)pre.w + ln;
            s = apply(t.map, s);
        }
    }
    __syncthreads();
    const uint32_t ti = (uint32_t)(total & 0xffffu), tb = (uint32_t)(total >> 16 & 0xffffu);
    for (uint32_t i = tid; i < ti; i += WG)
        ids[(uint64_t)pre.x + i] = tile_ids[i];
    for (uint32_t i = tid; i < tb; i += WG)
        bases[(uint64_t)pre.y + i] = tile_bases[i];
}

/* 6. the records without an id */
__global__ __launch_bounds__(256) void fq_parse_no_id_kernel(const uint64_t *__restrict__ id_offsets, uint32_t n_records,
                                                             uint64_t *sums)
{
    const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const bool empty = r < n_records && id_offsets[r + 1] == id_offsets[r];
    const uint64_t m = __ballot(empty);
    if ((threadIdx.x & 63u) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(&sums[SUM_NO_ID]), (unsigned long long)__popcll(m));
}

uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + SPAN - 1) / SPAN); }

/* count and sums over [0, n), and the sums read on the host */
int count_and_sum(kgx_ctx *c, const uint8_t *text, uint64_t n)
{
    hipStream_t st = c->stream;
    const uint32_t n_tiles = tiles_of(n);
    uint64_t *sums = c->fp_sum.as<uint64_t>();
    if (n_tiles)
        hipLaunchKernelGGL(fq_parse_count_kernel, dim3(n_tiles), dim3(WG), 0, st, text, n, c->fp_state.as<uint8_t>(),
                           c->fp_lane.as<uint8_t>(), c->fp_cnt.as<uint4>(), sums + SUM_ERROR_KEY);
    hipLaunchKernelGGL(fq_parse_sums_kernel, dim3(1), dim3(WG), 0, st, c->fp_cnt.as<uint4>(), n_tiles,
                       c->fp_pre.as<uint4>(), sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_fp_sum.data(), sums, (SUM_ERROR + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(host_wait(st));
    return KGX_OK;
}

/* kgx_fq_parse_device behind its argument checks; upload_ms is the caller's */
int fq_parse_device(kgx_ctx *c, const uint8_t *text, uint64_t n, uint32_t flags, kgx_fq_reads *out)
{
    hipStream_t st = c->stream;
    const uint32_t n_tiles = tiles_of(n);
    c->fq_parses++;
    HIP_TRY(c->fp_map.reserve((uint64_t)n_tiles * 4));
    HIP_TRY(c->fp_state.reserve((uint64_t)n_tiles + 1));
    HIP_TRY(c->fp_lane.reserve((uint64_t)n_tiles * WG));
    HIP_TRY(c->fp_cnt.reserve((uint64_t)n_tiles * 16));
    HIP_TRY(c->fp_pre.reserve((uint64_t)n_tiles * 16));
    HIP_TRY(c->fp_sum.reserve(SUM_WORDS * 8));
    HIP_TRY(c->h_fp_sum.resize(SUM_WORDS));
    uint64_t *sums = c->fp_sum.as<uint64_t>();
    uint64_t *h = c->h_fp_sum.data();
    HIP_TRY(hipEventRecord(c->fp_events[1], st));
    HIP_TRY(hipMemsetAsync(sums + SUM_ERROR_KEY, 0xff, 8, st));
    hipLaunchKernelGGL(fq_parse_map_kernel, dim3(n_tiles), dim3(WG), 0, st, text, n, c->fp_map.as<uint32_t>());
    hipLaunchKernelGGL(fq_parse_state_kernel, dim3(1), dim3(WG), 0, st, c->fp_map.as<uint32_t>(), n_tiles,
                       c->fp_state.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    if (int rc = count_and_sum(c, text, n))
        return rc;
    const uint64_t key = h[SUM_ERROR], all_newlines = h[SUM_NEWLINES];
    const bool offending = key != NO_ERROR;
    const uint64_t e = key >> 16;
    const bool cut = (flags & KGX_FQ_STRICT) && offending;
    uint64_t n_eff = n;
    if (cut) { /* the machine over [0, e) */
        n_eff = e;
        if (int rc = count_and_sum(c, text, n_eff))
            return rc;
    }
    const uint64_t n_ids = h[SUM_IDS], n_bases = h[SUM_BASES], n_rec = h[SUM_RECORDS], cut_newlines = h[SUM_NEWLINES];
    if (n_rec + 1 > UINT32_MAX || n_ids > n || n_bases > n)
        return fail(KGX_EDEVICE, "kgx_fq_parse: sums beyond what the text allows");
    HIP_TRY(c->fq_bases.reserve(n_bases + 16));
    HIP_TRY(c->fq_roff.reserve((n_rec + 2) * 8));
    HIP_TRY(c->ft_ids.reserve(n_ids + 16));
    HIP_TRY(c->ft_idoff.reserve((n_rec + 2) * 8));
    c->fq_up.active = false;
    c->fq_pend.active = false;
    hipLaunchKernelGGL(fq_parse_write_kernel, dim3(std::max<uint32_t>(1, tiles_of(n_eff))), dim3(WG), 0, st, text, n_eff,
                       c->fp_lane.as<uint8_t>(), c->fp_pre.as<uint4>(), (uint32_t)n_rec, n_ids, n_bases,
                       (offending && !cut) ? e : NO_ERROR, c->fq_bases.as<uint8_t>(), c->fq_roff.as<uint64_t>(),
                       c->ft_ids.as<uint8_t>(), c->ft_idoff.as<uint64_t>(), sums);
    if (n_rec)
        hipLaunchKernelGGL(fq_parse_no_id_kernel, dim3((uint32_t)((n_rec + WG - 1) / WG)), dim3(WG), 0, st,
                           c->ft_idoff.as<uint64_t>(), (uint32_t)n_rec, sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->fp_events[2], st));
    HIP_TRY(hipMemcpyAsync(h + SUM_CONSUMED, sums + SUM_CONSUMED, (SUM_NO_ID - SUM_CONSUMED + 1) * 8,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(host_wait(st));
    HIP_TRY(hipEventElapsedTime(&out->parse_ms, c->fp_events[1], c->fp_events[2]));

    /* the record in progress at the end of [0, n_eff) */
    const uint64_t tail_ids = n_ids - h[SUM_IDS_AT_END];
    bool tail = false;
    if (cut)
        tail = true;
    else if ((flags & KGX_FQ_STRICT) && (flags & KGX_FQ_FINISHED))
        tail = tail_ids != 0;
    out->n_reads = (uint32_t)(n_rec + tail);
    out->n_reads_no_id = (uint32_t)(h[SUM_NO_ID] + (tail && !tail_ids));
    out->n_bases = tail ? n_bases : h[SUM_BASES_AT_END];
    out->n_id_bytes = tail ? n_ids : h[SUM_IDS_AT_END];
    out->bases = c->fq_bases.as<uint8_t>();
    out->read_offsets = c->fq_roff.as<uint64_t>();
    out->ids = c->ft_ids.as<uint8_t>();
    out->id_offsets = c->ft_idoff.as<uint64_t>();
    const bool whole = (flags & KGX_FQ_STRICT) && (cut || (flags & KGX_FQ_FINISHED));
    out->consumed = whole ? n : h[SUM_CONSUMED];
    out->newlines = whole ? all_newlines : h[SUM_CONSUMED_NL];
    if (offending && (cut || e < out->consumed)) {
        out->error = (uint32_t)(key >> 8 & 255u);
        out->error_byte = (uint32_t)(key & 255u);
        out->error_pos = e;
        out->error_newlines = cut ? cut_newlines + (out->error_byte == '\n') : h[SUM_ERROR_NL];
    }
    return KGX_OK;
}

int parse_checks(kgx_ctx *c, const void *text, uint64_t n, uint32_t flags, kgx_fq_reads *out)
{
    if (!c || !out || (n && !text))
        return fail(KGX_EINVAL, "null argument");
    *out = kgx_fq_reads{};
    if (flags & ~(KGX_FQ_STRICT | KGX_FQ_FINISHED))
        return fail(KGX_EINVAL, "kgx_fq_parse: flags are KGX_FQ_STRICT and KGX_FQ_FINISHED");
    if (n > KGX_FQ_PARSE_MAX)
        return fail(KGX_ERANGE, "kgx_fq_parse: more than KGX_FQ_PARSE_MAX bytes of text in one call");
    HIP_TRY(hipSetDevice(c->img->device));
    return ensure_events(c->fp_events, 3, hipEventDefault);
}

}  // namespace

extern "C" {

int kgx_fq_parse_device(kgx_ctx *c, const void *d_text, uint64_t n, uint32_t flags, kgx_fq_reads *out)
{
    if (int rc = parse_checks(c, d_text, n, flags, out))
        return rc;
    if (!n)
        return KGX_OK;
    if (reinterpret_cast<uintptr_t>(d_text) & 15u)
        return fail(KGX_EINVAL, "kgx_fq_parse_device: d_text is not aligned to 16 bytes");
    return fq_parse_device(c, static_cast<const uint8_t *>(d_text), n, flags, out);
}

int kgx_fq_parse(kgx_ctx *c, const char *text, uint64_t n, uint32_t flags, kgx_fq_reads *out)
{
    if (int rc = parse_checks(c, text, n, flags, out))
        return rc;
    if (!n)
        return KGX_OK;
    hipStream_t st = c->stream;
    HIP_TRY(c->fp_text.reserve(n));
    const bool pinned = host_pinned_range(text, n);
    if (!pinned) {
        HIP_TRY(c->h_res.resize(n));
        parallel_memcpy(c->h_res.data(), text, n);
    }
    HIP_TRY(hipEventRecord(c->fp_events[0], st));
    HIP_TRY(hipMemcpyAsync(c->fp_text.p, pinned ? static_cast<const void *>(text) : c->h_res.data(), n,
                           hipMemcpyHostToDevice, st));
    if (int rc = fq_parse_device(c, c->fp_text.as<uint8_t>(), n, flags, out))
        return rc;
    HIP_TRY(hipEventElapsedTime(&out->upload_ms, c->fp_events[0], c->fp_events[1]));
    return KGX_OK;
}

}  // extern "C"
