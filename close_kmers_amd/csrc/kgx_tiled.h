/*
 * kgx_tiled.h -- a context's tiled device hits, enumerated per (tile, hit)
 * in either hit format: the view the k-mer tables (kgx_tables.hip) and the
 * grouping by k-mer set (kgx_uniq.hip) read the hit stream through.
 */
#ifndef KGX_TILED_H
#define KGX_TILED_H

#include "kgx_device.h"
#include "kgx_rt.h"

namespace kgx {

/* the tiled device result of a context (kgx_device_result) */
struct Tiled {
    const uint4 *hot;  /* the hit records (HIT_PACKED16) or plane 0 */
    const uint4 *cold; /* HIT_PLANES: {which_kmer lo, hi, otu, seq} per slot */
    const uint64_t *mask;
    const uint64_t *wbase;
    const uint32_t *tile_seq;
    uint32_t n_seq;
    uint32_t T; /* windows per tile */
    bool packed;
};

/* k-mer and sequence of hit i of `tile` */
__device__ __forceinline__ void hit_key_seq(const Tiled &t, uint64_t tile, uint32_t i, uint64_t &key, uint32_t &seq)
{
    const uint64_t slot = tile * t.T + i;
    if (t.packed) {
        key = HitFields<true>::key(t.hot[slot], t.hot[slot]);
        seq = window_seq(t.wbase, t.tile_seq, tile, hit_window(t.mask, tile, t.T / 64, i));
    } else {
        const uint4 h = t.cold[slot];
        key = (uint64_t)h.y << 32 | h.x;
        seq = h.w;
    }
}

__device__ __forceinline__ uint64_t hit_key(const Tiled &t, uint64_t tile, uint32_t i)
{
    const uint64_t slot = tile * t.T + i;
    if (t.packed)
        return HitFields<true>::key(t.hot[slot], t.hot[slot]);
    const uint4 h = t.cold[slot];
    return (uint64_t)h.y << 32 | h.x;
}

__device__ __forceinline__ uint32_t tile_count(const Tiled &t, uint64_t tile)
{
    const uint64_t W = t.wbase[t.n_seq];
    const uint32_t J = t.T / 64;
    uint32_t c = 0;
    for (uint32_t j = 0; j < J; j++) {
        const uint64_t w = tile * J + j;
        if (64 * w < W)
            c += (uint32_t)__popcll(t.mask[w]);
    }
    return c;
}

/* the view of c's planned batch, once a probe has left its hits (c->have_hits) */
inline Tiled tiled_of(const kgx_ctx *c)
{
    Tiled t;
    t.hot = c->hits.as<uint4>();
    t.cold = c->hits.as<uint4>() + c->hit_slots;
    t.mask = c->hit_mask.as<uint64_t>();
    t.wbase = c->wbase.as<uint64_t>();
    t.tile_seq = c->tile_seq.as<uint32_t>();
    t.n_seq = c->n_seq;
    t.T = c->tile_windows;
    t.packed = c->hit_format == HIT_PACKED16;
    return t;
}

}  // namespace kgx

#endif
