/*
 * kgx_text_scan.h -- a byte-at-a-time text parser as scanned state maps, for
 * the device: what kgx_fq_parse.hip and kgx_fa_parse.hip
 * (§8.13) share.  Device code only; both files instantiate it with their
 * machine.
 *
 * What a byte does depends on the state before it, so a run of bytes is a map
 * from entry state to exit state: N_STATES x 3 bits in one word, and maps
 * compose associatively.  A machine M gives
 *
 *   N_STATES, N_CLASSES     at most 8 states (3 bits each, 4 event bits each);
 *                           state 0 is the start state, the last class is the
 *                           one every byte without a rule of its own falls in
 *   C_NL                    the class of '\n' (counted: the line of an error)
 *   END_TAKES_BYTE          1: the byte that ends a record is the record's
 *                           last, 0: it is the next record's first
 *   next_state(s, c)        constexpr: the state after a byte of class c in s
 *   event_of(s, c)          constexpr: EV_ID | EV_DATA | EV_END | EV_BAD
 *   class_of(b)             the byte's class
 *   error_code(s, b)        the code of byte b offending in state s
 *
 * and the kernels are, per 4096-byte tile (256 lanes x 16 bytes as one uint4):
 *
 *   map    a lane builds the map of its 16 bytes, the wave composes by
 *          shuffles, the workgroup through LDS: one map per tile
 *   state  one workgroup scans the tile maps: the entry state of every tile
 *   count  with the entry state known, per lane its entry state (kept, one
 *          byte), per tile the id bytes, data bytes, record ends and newlines,
 *          and the first offending byte (one atomicMin per tile that has one)
 *   sums   one workgroup: the exclusive sums of the tiles' counts, the totals
 *   write  id bytes and data bytes compacted through LDS to their places; the
 *          lane that sees record end k writes data_offsets[k + 1] and
 *          id_offsets[k + 1]
 *   no_id  the records without an id, counted
 *
 * Separate launches: no kernel waits on another workgroup.
 */
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kgx {
namespace text_scan {

constexpr uint32_t SPAN = 4096; /* bytes per workgroup: 256 lanes x 16 */
constexpr uint32_t LANE_BYTES = 16;
constexpr uint32_t WG = 256, WAVES = 4;

enum : uint32_t { EV_ID = 1, EV_DATA = 2, EV_END = 4, EV_BAD = 8 };

constexpr uint32_t NL_BIT = 1u << 31; /* in a byte's map word: the byte is '\n' */
constexpr uint64_t NO_ERROR = ~0ull;  /* the error key: pos << 16 | code << 8 | byte */

/* the sums a call leaves for the host, uint64 each */
enum : uint32_t {
    SUM_IDS, SUM_DATA, SUM_RECORDS, SUM_NEWLINES, SUM_ERROR, /* after the sums kernel */
    SUM_CONSUMED = 8, SUM_CONSUMED_NL, SUM_IDS_AT_END, SUM_DATA_AT_END, SUM_ERROR_NL, SUM_NO_ID, /* after write */
    SUM_ERROR_KEY = 15, /* the count kernel's atomicMin */
    SUM_WORDS
};

/* class c as a map: state s -> bits [3s, 3s + 3) */
template <class M> constexpr uint32_t map_word(uint32_t c)
{
    uint32_t w = 0;
    for (uint32_t s = 0; s < M::N_STATES; s++)
        w |= M::next_state(s, c) << (3 * s);
    return w;
}

/* class c's events: state s -> bits [4s, 4s + 4) */
template <class M> constexpr uint32_t event_word(uint32_t c)
{
    uint32_t w = 0;
    for (uint32_t s = 0; s < M::N_STATES; s++)
        w |= M::event_of(s, c) << (4 * s);
    return w;
}

template <class M> constexpr uint32_t identity()
{
    uint32_t w = 0;
    for (uint32_t s = 0; s < M::N_STATES; s++)
        w |= s << (3 * s);
    return w;
}

struct ByteWords {
    uint32_t map, events;
};

/* the words of class C when c is C, for every class but the last */
template <class M, uint32_t C> __device__ __forceinline__ void class_words(uint32_t c, uint32_t &m, uint32_t &e)
{
    if constexpr (C + 1 < M::N_CLASSES) {
        m = c == C ? (map_word<M>(C) | (C == M::C_NL ? NL_BIT : 0u)) : m;
        e = c == C ? event_word<M>(C) : e;
        class_words<M, C + 1>(c, m, e);
    }
}

/* the byte's map and event words: tab[b], filled by the workgroup's 256 lanes */
template <class M> __device__ __forceinline__ void fill_table(ByteWords *tab, uint32_t tid)
{
    const uint32_t c = M::class_of(tid);
    uint32_t m = map_word<M>(M::N_CLASSES - 1), e = event_word<M>(M::N_CLASSES - 1);
    class_words<M, 0>(c, m, e);
    tab[tid].map = m;
    tab[tid].events = e;
}

/* f, then g: (g o f)(s) for every s */
template <class M> __device__ __forceinline__ uint32_t then(uint32_t f, uint32_t g)
{
    uint32_t r = 0;
#pragma unroll
    for (uint32_t s = 0; s < M::N_STATES; s++)
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
template <class M> __device__ __forceinline__ uint32_t lane_map(const ByteWords *tab, const uint32_t (&w)[4], uint32_t valid)
{
    uint32_t m = identity<M>();
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++)
        if (j < valid)
            m = then<M>(m, tab[byte_of(w, j)].map);
    return m;
}

/* inclusive composition over the wave's lanes, lane 0 first */
template <class M> __device__ __forceinline__ uint32_t wave_scan_maps(uint32_t m, uint32_t lane)
{
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(m, d, 64);
        if (lane >= d)
            m = then<M>(o, m);
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
template <class M>
__device__ __forceinline__ void map_body(const uint8_t *__restrict__ text, uint64_t n, uint32_t *__restrict__ tile_map)
{
    __shared__ ByteWords tab[256];
    __shared__ uint32_t wave_map[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table<M>(tab, tid);
    __syncthreads();
    uint32_t w[4];
    const uint32_t valid = load_lane(text, n, (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES, w);
    const uint32_t inc = wave_scan_maps<M>(lane_map<M>(tab, w, valid), lane);
    if (lane == 63)
        wave_map[wv] = inc;
    __syncthreads();
    if (tid == 0)
        tile_map[blockIdx.x] = then<M>(then<M>(then<M>(wave_map[0], wave_map[1]), wave_map[2]), wave_map[3]);
}

/* 2. one workgroup: every tile's entry state, and the text's end state in
 * tile_state[n_tiles] */
template <class M>
__device__ __forceinline__ void state_body(const uint32_t *__restrict__ tile_map, uint32_t n_tiles,
                                           uint8_t *__restrict__ tile_state)
{
    __shared__ uint32_t wave_map[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_tiles; base += WG) {
        const uint32_t i = base + tid;
        const uint32_t inc = wave_scan_maps<M>(i < n_tiles ? tile_map[i] : identity<M>(), lane);
        if (lane == 63)
            wave_map[wv] = inc;
        __syncthreads();
        uint32_t exc = __shfl_up(inc, 1, 64);
        if (lane == 0)
            exc = identity<M>();
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
template <class M>
__device__ __forceinline__ uint32_t lane_entry_state(uint32_t m, uint32_t tile_entry, uint32_t *wave_map, uint32_t lane,
                                                     uint32_t wv)
{
    const uint32_t inc = wave_scan_maps<M>(m, lane);
    if (lane == 63)
        wave_map[wv] = inc;
    __syncthreads();
    uint32_t exc = __shfl_up(inc, 1, 64);
    if (lane == 0)
        exc = identity<M>();
    uint32_t s = tile_entry;
    for (uint32_t k = 0; k < wv; k++)
        s = apply(wave_map[k], s);
    return apply(exc, s);
}

/* id bytes | data bytes << 16 | record ends << 32 | newlines << 48: a tile has
 * 4096 bytes, so no field carries into the next */
__device__ __forceinline__ uint64_t pack_counts(uint32_t ids, uint32_t data, uint32_t ends, uint32_t nls)
{
    return (uint64_t)ids | (uint64_t)data << 16 | (uint64_t)ends << 32 | (uint64_t)nls << 48;
}

/* 3. the lanes' entry states, the tile's counts, the first offending byte */
template <class M>
__device__ __forceinline__ void count_body(const uint8_t *__restrict__ text, uint64_t n,
                                           const uint8_t *__restrict__ tile_state, uint8_t *__restrict__ lane_state,
                                           uint4 *__restrict__ tile_cnt, uint64_t *error_key)
{
    __shared__ ByteWords tab[256];
    __shared__ uint32_t wave_map[WAVES];
    __shared__ uint64_t wave_cnt[WAVES];
    __shared__ unsigned long long tile_key;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table<M>(tab, tid);
    if (tid == 0)
        tile_key = NO_ERROR;
    __syncthreads();
    uint32_t w[4];
    const uint64_t pos = (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES;
    const uint32_t valid = load_lane(text, n, pos, w);
    uint32_t s = lane_entry_state<M>(lane_map<M>(tab, w, valid), tile_state[blockIdx.x], wave_map, lane, wv);
    lane_state[(uint64_t)blockIdx.x * WG + tid] = (uint8_t)s;
    uint32_t ids = 0, data = 0, ends = 0, nls = 0;
    uint64_t key = NO_ERROR;
#pragma unroll
    for (uint32_t j = 0; j < LANE_BYTES; j++) {
        if (j < valid) {
            const uint32_t b = byte_of(w, j);
            const ByteWords t = tab[b];
            const uint32_t ev = (t.events >> (4u * s)) & 15u;
            ids += ev & 1u;
            data += (ev >> 1) & 1u;
            ends += (ev >> 2) & 1u;
            nls += t.map >> 31;
            if ((ev & EV_BAD) && key == NO_ERROR) {
                const uint32_t code = M::error_code(s, b);
                key = (pos + j) << 16 | (uint64_t)code << 8 | b;
            }
            s = apply(t.map, s);
        }
    }
    if (key != NO_ERROR)
        atomicMin(&tile_key, (unsigned long long)key);
    uint64_t c = pack_counts(ids, data, ends, nls);
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

/* 4. one workgroup: the exclusive sums of the tiles' counts (x ids, y data
 * bytes, z record ends, w newlines; a text of at most 0xFFFFF000 bytes keeps
 * them in 32 bits) and the call's sums.  The same for every machine. */
__device__ __forceinline__ void sums_body(const uint4 *__restrict__ tile_cnt, uint32_t n_tiles,
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
        sums[SUM_DATA] = carry.y;
        sums[SUM_RECORDS] = carry.z;
        sums[SUM_NEWLINES] = carry.w;
        sums[SUM_ERROR] = sums[SUM_ERROR_KEY];
    }
    if (tid >= SUM_CONSUMED && tid <= SUM_NO_ID)
        sums[tid] = 0;
}

/* 5. the outputs.  grid = max(1, tiles of [0, n)); n_records, n_ids and
 * n_data are the sums over [0, n).  data_offsets and id_offsets hold
 * n_records + 2 entries: [0] = 0, one per record end, and the record in
 * progress at n closed by the totals (the host decides whether it is a
 * record).  error_pos: the byte whose newline count the host wants (NO_ERROR:
 * none) */
template <class M>
__device__ __forceinline__ void write_body(const uint8_t *__restrict__ text, uint64_t n,
                                           const uint8_t *__restrict__ lane_state, const uint4 *__restrict__ tile_pre,
                                           uint32_t n_records, uint64_t n_ids, uint64_t n_data, uint64_t error_pos,
                                           uint8_t *__restrict__ data, uint64_t *__restrict__ data_offsets,
                                           uint8_t *__restrict__ ids, uint64_t *__restrict__ id_offsets, uint64_t *sums)
{
    __shared__ ByteWords tab[256];
    __shared__ uint64_t wave_cnt[WAVES];
    __shared__ uint8_t tile_ids[SPAN], tile_data[SPAN];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    fill_table<M>(tab, tid);
    if (blockIdx.x == 0 && tid == 0) {
        data_offsets[0] = 0;
        id_offsets[0] = 0;
        data_offsets[(uint64_t)n_records + 1] = n_data;
        id_offsets[(uint64_t)n_records + 1] = n_ids;
    }
    __syncthreads();
    uint32_t w[4];
    const uint64_t pos = (uint64_t)blockIdx.x * SPAN + tid * LANE_BYTES;
    const uint32_t valid = load_lane(text, n, pos, w);
    const uint32_t s0 = valid ? lane_state[(uint64_t)blockIdx.x * WG + tid] : 0u;
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
            if (ev & EV_DATA)
                tile_data[lb++] = (uint8_t)b;
            ln += t.map >> 31;
            if (ev & EV_END) {
                const uint64_t k = (uint64_t)pre.z + le++;
                data_offsets[k + 1] = (uint64_t)pre.y + lb;
                id_offsets[k + 1] = (uint64_t)pre.x + li;
                if (k + 1 == n_records) { /* the last record's end: what the caller has consumed */
                    sums[SUM_CONSUMED] = pos + j + M::END_TAKES_BYTE;
                    sums[SUM_CONSUMED_NL] = (uint64_t)pre.w + ln;
                    sums[SUM_IDS_AT_END] = (uint64_t)pre.x + li;
                    sums[SUM_DATA_AT_END] = (uint64_t)pre.y + lb;
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
        data[(uint64_t)pre.y + i] = tile_data[i];
}

/* 6. the records without an id */
__device__ __forceinline__ void no_id_body(const uint64_t *__restrict__ id_offsets, uint32_t n_records, uint64_t *sums)
{
    const uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x;
    const bool empty = r < n_records && id_offsets[r + 1] == id_offsets[r];
    const uint64_t m = __ballot(empty);
    if ((threadIdx.x & 63u) == 0 && m)
        atomicAdd(reinterpret_cast<unsigned long long *>(&sums[SUM_NO_ID]), (unsigned long long)__popcll(m));
}

inline uint32_t tiles_of(uint64_t n) { return (uint32_t)((n + SPAN - 1) / SPAN); }

}  // namespace text_scan
}  // namespace kgx
