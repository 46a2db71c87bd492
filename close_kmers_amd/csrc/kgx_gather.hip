/*
 * kgx_gather.hip -- the last step of the lookup path and what brings its
 * results to the host.
 *
 *   gather : tiled hits -> dense per-sequence CSR (host-buffer path), with
 *            the count scan that gives the CSR offsets; the small-batch
 *            upload and collectors; the device -> mapped host copy kernels
 */
#include "kgx_device.h"
#include "kgx_lstd.h"

namespace kgx {

/* ------------------------------------------------------------------------ */
/* gather: tiled hits / sparse calls -> dense CSR, one wave per sequence     */
/* ------------------------------------------------------------------------ */

constexpr uint32_t CS_PER = 4, CS_TILE = 256 * CS_PER;

struct Counts3 {
    const uint32_t *c[3]; /* NULL: an all-zero array */
};
struct Offsets3 {
    uint64_t *o[3];
};

/* sequence s's records, by one wave, to its dense CSR slots (hits from hoff_s,
 * calls from coff_s, OTUs from ooff_s; each read only for the outputs asked) */
template <bool PK>
__device__ __forceinline__ void gather_one(
    uint32_t s, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, const uint32_t *__restrict__ call_count, const uint4 *__restrict__ hot,
    const uint4 *__restrict__ cold, const kgx_call *__restrict__ calls, uint64_t hoff_s, uint64_t coff_s,
    kgx_hit *__restrict__ hits_out, kgx_call *__restrict__ calls_out, uint32_t seq_base,
    const uint32_t *__restrict__ otu_count, const kgx_otu *__restrict__ otus, uint64_t ooff_s,
    kgx_otu *__restrict__ otus_out, uint4 *__restrict__ hits16_out, uint32_t *__restrict__ hits12_out)
{
    const uint32_t lane = lane_id();
    const uint64_t gw0 = wbase[s], gw1 = wbase[s + 1];
    if ((hits_out || (PK && (hits16_out || hits12_out))) && gw0 < gw1) {
        const uint32_t J = tile_windows / 64;
        const uint64_t gfirst = gw0 >> 6, glast = (gw1 - 1) >> 6;
        uint64_t done = 0; /* hits of s written so far */
        for (uint64_t gb = gfirst; gb <= glast; gb += 64) {
            /* lane l takes mask word gb + l: its run inside the tile */
            const uint64_t g = gb + lane;
            uint64_t at = 0, bits = 0;
            uint32_t cnt = 0;
            if (g <= glast) {
                const uint64_t tile = g / J;
                uint32_t pre = 0;
                for (uint64_t x = tile * J; x < g; x++)
                    pre += (uint32_t)__popcll(hit_mask[x]);
                const uint64_t full = hit_mask[g];
                const uint32_t lo = g == gfirst ? (uint32_t)(gw0 & 63) : 0u;
                const uint32_t hi = g == glast ? (uint32_t)((gw1 - 1) & 63) + 1 : 64u;
                bits = full & bit_range(lo, hi);
                cnt = (uint32_t)__popcll(bits);
                at = tile * tile_windows + pre + (uint32_t)__popcll(full & bit_range(0, lo));
            }
            /* exclusive prefix of cnt over the wave */
            uint32_t incl = cnt;
            for (uint32_t off = 1; off < 64; off <<= 1) {
                const uint32_t x = __shfl_up(incl, off);
                if (lane >= off)
                    incl += x;
            }
            const uint64_t dst0 = hoff_s + done + (incl - cnt);
            /* a lane's run is read GB records at a time, all in flight before
             * any is stored (a load-store loop would wait on every record) */
            constexpr uint32_t GB = 4;
            if (PK && hits16_out) { /* the records as stored: position = mask bit */
                for (uint32_t i0 = 0; i0 < cnt; i0 += GB) {
                    uint4 h[GB];
#pragma unroll
                    for (uint32_t k = 0; k < GB; k++)
                        if (i0 + k < cnt)
                            h[k] = hot[at + i0 + k];
#pragma unroll
                    for (uint32_t k = 0; k < GB; k++)
                        if (i0 + k < cnt)
                            hits16_out[dst0 + i0 + k] = h[k];
                }
                done += __shfl(incl, 63);
                continue;
            }
            if (PK && hits12_out) { /* the records less the key (the host re-encodes it) */
                for (uint32_t i0 = 0; i0 < cnt; i0 += GB) {
                    uint4 h[GB];
#pragma unroll
                    for (uint32_t k = 0; k < GB; k++)
                        if (i0 + k < cnt)
                            h[k] = hot[at + i0 + k];
#pragma unroll
                    for (uint32_t k = 0; k < GB; k++)
                        if (i0 + k < cnt) {
                            uint32_t *d = hits12_out + 3 * (dst0 + i0 + k);
                            d[0] = h[k].z;      /* function_wt bits */
                            d[1] = h[k].w;      /* avg_from_end | (otu+1) high 12 << 16 | flags << 28 */
                            d[2] = h[k].y >> 3; /* (fI+1) | (otu+1) low 9 << 20: packed lo >> 35 */
                        }
                }
                done += __shfl(incl, 63);
                continue;
            }
            uint4 *dst = reinterpret_cast<uint4 *>(hits_out + dst0);
            const uint32_t pbase = (uint32_t)(64 * g - gw0);
            for (uint32_t i0 = 0; i0 < cnt; i0 += GB) { /* kgx_hit from its record(s) */
                uint4 h[GB], c[GB];
#pragma unroll
                for (uint32_t k = 0; k < GB; k++)
                    if (i0 + k < cnt) {
                        h[k] = hot[at + i0 + k];
                        if (!PK)
                            c[k] = cold[at + i0 + k];
                    }
#pragma unroll
                for (uint32_t k = 0; k < GB; k++) {
                    if (i0 + k >= cnt)
                        break;
                    const uint32_t i = i0 + k;
                    const uint32_t pos = pbase + (uint32_t)__builtin_ctzll(bits);
                    bits &= bits - 1;
                    if (PK) {
                        typedef HitFields<true> HF;
                        const uint64_t key = HF::key(h[k], h[k]);
                        dst[2 * i] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), HF::otu(h[k], h[k]),
                                                HF::avg(h[k]) | HF::flags(h[k]) << 16);
                        dst[2 * i + 1] = make_uint4(HF::fi(h[k]), HF::wt(h[k]), pos, s + seq_base);
                    } else {
                        dst[2 * i] = make_uint4(c[k].x, c[k].y, c[k].z, h[k].x);
                        dst[2 * i + 1] = make_uint4(h[k].y, h[k].z, pos, s + seq_base);
                    }
                }
            }
            done += __shfl(incl, 63);
        }
    }
    if (calls_out) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(calls + gw0);
        uint32_t *dst = reinterpret_cast<uint32_t *>(calls_out + coff_s);
        const uint32_t n = 5 * call_count[s];
        for (uint32_t i = lane; i < n; i += 64)
            dst[i] = src[i];
    }
    if (otus_out) {
        const kgx_otu *src = otus + gw0;
        kgx_otu *dst = otus_out + ooff_s;
        for (uint32_t i = lane; i < otu_count[s]; i += 64)
            dst[i] = src[i];
    }
}

template <bool PK>
__global__ __launch_bounds__(256) void gather_kernel(
    uint32_t n_seq, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, const uint32_t *__restrict__ call_count, const uint4 *__restrict__ hot,
    const uint4 *__restrict__ cold, const kgx_call *__restrict__ calls, const uint64_t *__restrict__ hoff,
    const uint64_t *__restrict__ coff, kgx_hit *__restrict__ hits_out, kgx_call *__restrict__ calls_out,
    uint32_t seq_base, const uint32_t *__restrict__ otu_count, const kgx_otu *__restrict__ otus,
    const uint64_t *__restrict__ ooff, kgx_otu *__restrict__ otus_out, uint4 *__restrict__ hits16_out,
    uint32_t *__restrict__ hits12_out)
{
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= n_seq)
        return;
    const bool want_hits = hits_out || (PK && (hits16_out || hits12_out));
    gather_one<PK>(s, wbase, hit_mask, tile_windows, call_count, hot, cold, calls, want_hits ? hoff[s] : 0,
                   calls_out ? coff[s] : 0, hits_out, calls_out, seq_base, otu_count, otus,
                   otus_out ? ooff[s] : 0, otus_out, hits16_out, hits12_out);
}

/* small batches (<= SMALL_GATHER_SEQ sequences): small_collect and gather in
 * one launch -- every workgroup scans the counts into LDS (workgroup 0 also
 * into the caller's mapped offsets), then its four waves gather sequences
 * 4 b .. 4 b + 3 from those offsets (SMALL_GATHER_BLOCKS workgroups at most,
 * striding); the workgroup that finishes last (a device counter, reset by
 * it) stores the token */
template <bool PK>
__global__ __launch_bounds__(256) void small_gather_kernel(
    uint32_t n, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask, uint32_t tile_windows,
    const uint32_t *__restrict__ hit_count, const uint32_t *__restrict__ call_count, const uint4 *__restrict__ hot,
    const uint4 *__restrict__ cold, const kgx_call *__restrict__ calls, const uint32_t *__restrict__ otu_count,
    const kgx_otu *__restrict__ otus, kgx_hit *__restrict__ hits_out, kgx_call *__restrict__ calls_out,
    kgx_otu *__restrict__ otus_out, Offsets3 off_host, const uint32_t *__restrict__ status,
    const kgx_best_call *__restrict__ best, kgx_best_call *__restrict__ best_host, uint32_t *__restrict__ status_host,
    uint64_t *__restrict__ nwin_host, uint32_t *done_host, uint32_t token, uint32_t *blocks_done)
{
    __shared__ uint64_t lds4[3][4];
    __shared__ uint64_t lo[3][SMALL_GATHER_SEQ + 1];
    __shared__ uint32_t last;
    const uint32_t t = threadIdx.x;
    const bool first = blockIdx.x == 0;
    const uint32_t *cnt[3] = {hit_count, calls_out ? call_count : nullptr, otus_out ? otu_count : nullptr};
    for (int a = 0; a < 3; a++) {
        const uint64_t v = t < n && cnt[a] ? cnt[a][t] : 0;
        uint64_t tot;
        const uint64_t ex = block_scan(v, lds4[a], tot) - v;
        if (t < n) {
            lo[a][t] = ex;
            if (first)
                off_host.o[a][t] = ex;
        }
        if (t == 0) {
            lo[a][n] = tot;
            if (first)
                off_host.o[a][n] = tot;
        }
    }
    if (first && best_host && t < n)
        best_host[t] = best[t];
    if (first && t == 0) {
        status_host[0] = status[0];
        nwin_host[0] = wbase[n];
    }
    __syncthreads();
    for (uint32_t s = blockIdx.x * 4 + (t >> 6); s < n; s += 4 * gridDim.x)
        gather_one<PK>(s, wbase, hit_mask, tile_windows, call_count, hot, cold, calls, lo[0][s], lo[1][s], hits_out,
                       calls_out, 0u, otu_count, otus, lo[2][s], otus_out, nullptr, nullptr);
    /* the batch's last word: every store above, of every workgroup, is
     * visible to the host before the host sees done_host == token (it polls
     * instead of a stream sync) */
    if (done_host) {
        __threadfence_system();
        __syncthreads();
        if (t == 0) {
            last = gridDim.x == 1 || atomicAdd(blocks_done, 1u) == gridDim.x - 1;
            if (last && gridDim.x > 1)
                *blocks_done = 0; /* for the next launch on this stream */
        }
        __syncthreads();
        if (t == 0 && last) {
            __threadfence_system();
            *reinterpret_cast<volatile uint32_t *>(done_host) = token;
        }
    }
}

hipError_t launch_small_gather(uint32_t n, const uint64_t *wbase, const uint64_t *hit_mask, uint32_t tile_windows,
                               const uint32_t *hit_count, const uint32_t *call_count, const uint4 *hot,
                               const uint4 *cold, const kgx_call *calls, const uint32_t *otu_count,
                               const kgx_otu *otus, kgx_hit *hits_out, kgx_call *calls_out, kgx_otu *otus_out,
                               uint64_t *h0, uint64_t *h1, uint64_t *h2, const uint32_t *status,
                               const kgx_best_call *best, kgx_best_call *best_host, uint32_t *status_host,
                               uint64_t *nwin_host, uint32_t *done_host, uint32_t token, uint32_t *blocks_done,
                               uint32_t hit_format, hipStream_t stream)
{
    if (n == 0 || n > SMALL_GATHER_SEQ)
        return hipErrorInvalidValue;
    const Offsets3 off_host = {{h0, h1, h2}};
    /* one wave per sequence (blocks_done NULL: one workgroup) */
    const uint32_t blocks = blocks_done ? std::min<uint32_t>((n + 3) / 4, SMALL_GATHER_BLOCKS) : 1u;
    if (hit_format == HIT_PACKED16)
        hipLaunchKernelGGL(small_gather_kernel<true>, dim3(blocks), dim3(256), 0, stream, n, wbase, hit_mask,
                           tile_windows, hit_count, call_count, hot, cold, calls, otu_count, otus, hits_out, calls_out,
                           otus_out, off_host, status, best, best_host, status_host, nwin_host, done_host, token,
                           blocks_done);
    else
        hipLaunchKernelGGL(small_gather_kernel<false>, dim3(blocks), dim3(256), 0, stream, n, wbase, hit_mask,
                           tile_windows, hit_count, call_count, hot, cold, calls, otu_count, otus, hits_out,
                           calls_out, otus_out, off_host, status, best, best_host, status_host, nwin_host,
                           done_host, token, blocks_done);
    return hipGetLastError();
}

hipError_t launch_gather(uint32_t n_seq, const uint64_t *wbase, const uint64_t *hit_mask,
                         uint32_t tile_windows, const uint32_t *call_count, const uint4 *hot, const uint4 *cold,
                         const kgx_call *calls, const uint64_t *hoff, const uint64_t *coff,
                         kgx_hit *hits_out, kgx_call *calls_out, uint32_t seq_base, uint32_t hit_format,
                         const uint32_t *otu_count, const kgx_otu *otus, const uint64_t *ooff, kgx_otu *otus_out,
                         hipStream_t stream, uint4 *hits16_out, uint32_t *hits12_out)
{
    if (n_seq == 0)
        return hipSuccess;
    if (hit_format == HIT_PACKED16)
        hipLaunchKernelGGL(gather_kernel<true>, dim3((n_seq + 3) / 4), dim3(256), 0, stream, n_seq, wbase,
                           hit_mask, tile_windows, call_count, hot, cold, calls, hoff, coff, hits_out,
                           calls_out, seq_base, otu_count, otus, ooff, otus_out, hits16_out, hits12_out);
    else
        hipLaunchKernelGGL(gather_kernel<false>, dim3((n_seq + 3) / 4), dim3(256), 0, stream, n_seq, wbase,
                           hit_mask, tile_windows, call_count, hot, cold, calls, hoff, coff, hits_out,
                           calls_out, seq_base, otu_count, otus, ooff, otus_out, hits16_out, hits12_out);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* count scan: a chunk's dense CSR offsets from its per-sequence counts, on  */
/* the device (the streamed host path needs no host round trip between the  */
/* scorer and the gather): off[a][i] = sum_{j<i} count[a][j], i in [0, n]   */
/* ------------------------------------------------------------------------ */


__device__ __forceinline__ uint64_t thread_count(const uint32_t *c, uint32_t n, uint32_t i0)
{
    uint64_t v = 0;
    if (c)
        for (uint32_t k = 0; k < CS_PER; k++)
            if (i0 + k < n)
                v += c[i0 + k];
    return v;
}

__global__ __launch_bounds__(256) void count_reduce_kernel(Counts3 cnt, uint32_t n, uint64_t *__restrict__ sums)
{
    __shared__ uint64_t lds4[3][4];
    const uint32_t i0 = blockIdx.x * CS_TILE + threadIdx.x * CS_PER;
    for (int a = 0; a < 3; a++) {
        uint64_t total;
        block_scan(thread_count(cnt.c[a], n, i0), lds4[a], total);
        if (threadIdx.x == 0)
            sums[3 * (uint64_t)blockIdx.x + a] = total;
    }
}

/* exclusive scan of the 3 x groups workgroup sums in place, one workgroup */
__global__ __launch_bounds__(256) void count_sums_scan_kernel(uint64_t *__restrict__ sums, uint32_t groups)
{
    __shared__ uint64_t lds4[3][4];
    uint64_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < groups; base += 256) {
        const uint32_t i = base + threadIdx.x;
        for (int a = 0; a < 3; a++) {
            const uint64_t v = i < groups ? sums[3 * (uint64_t)i + a] : 0;
            uint64_t tot;
            const uint64_t incl = block_scan(v, lds4[a], tot);
            if (i < groups)
                sums[3 * (uint64_t)i + a] = carry[a] + incl - v;
            carry[a] += tot;
        }
        __syncthreads(); /* lds4 is rewritten by the next round */
    }
}

__global__ __launch_bounds__(256) void count_scan_kernel(Counts3 cnt, uint32_t n, const uint64_t *__restrict__ sums,
                                                         Offsets3 off)
{
    __shared__ uint64_t lds4[3][4];
    const uint32_t i0 = blockIdx.x * CS_TILE + threadIdx.x * CS_PER;
    for (int a = 0; a < 3; a++) {
        uint64_t tot;
        const uint64_t mine = thread_count(cnt.c[a], n, i0);
        uint64_t at = sums[3 * (uint64_t)blockIdx.x + a] + block_scan(mine, lds4[a], tot) - mine;
        /* entries [i0, i0 + CS_PER) of the n + 1 offsets */
        for (uint32_t k = 0; k < CS_PER && i0 + k <= n; k++) {
            off.o[a][i0 + k] = at;
            if (cnt.c[a] && i0 + k < n)
                at += cnt.c[a][i0 + k];
        }
    }
}

size_t count_scan_workspace_bytes(uint32_t n)
{
    return (size_t)3 * ((n + 1 + CS_TILE - 1) / CS_TILE) * sizeof(uint64_t);
}

hipError_t launch_count_scan(uint32_t n, const uint32_t *c0, const uint32_t *c1, const uint32_t *c2, uint64_t *o0,
                             uint64_t *o1, uint64_t *o2, void *workspace, hipStream_t stream)
{
    const uint32_t groups = (n + 1 + CS_TILE - 1) / CS_TILE; /* n + 1 offsets */
    Counts3 cnt = {{c0, c1, c2}};
    Offsets3 off = {{o0, o1, o2}};
    uint64_t *sums = static_cast<uint64_t *>(workspace);
    hipLaunchKernelGGL(count_reduce_kernel, dim3(groups), dim3(256), 0, stream, cnt, n, sums);
    hipLaunchKernelGGL(count_sums_scan_kernel, dim3(1), dim3(256), 0, stream, sums, groups);
    hipLaunchKernelGGL(count_scan_kernel, dim3(groups), dim3(256), 0, stream, cnt, n,
                       static_cast<const uint64_t *>(sums), off);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* small batches (one or a few sequences, e.g. the facade's process_aa_seq): */
/* the host plans the batch itself and the device reads it from mapped      */
/* pinned memory, and the counts are scanned and the results land in mapped */
/* memory too, so a batch costs one host wait and no DMA copies             */
/* ------------------------------------------------------------------------ */

/* pieces of mapped pinned host memory -> HBM: one 16-B load per thread over
 * the pieces' concatenation (one PCIe round trip for a small batch) */
__global__ __launch_bounds__(256) void small_upload_kernel(SmallPieces pc)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pc.end16[SMALL_PIECES - 1];
         i += stride) {
        int p = 0;
#pragma unroll
        for (int k = 0; k < SMALL_PIECES - 1; k++)
            p += i >= pc.end16[k];
        const uint64_t j = i - (p ? pc.end16[p - 1] : 0);
        pc.dst[p][j] = pc.src[p][j];
    }
}

hipError_t launch_small_upload(const SmallPieces &pc, hipStream_t stream)
{
    const uint64_t n16 = pc.end16[SMALL_PIECES - 1];
    if (n16 == 0)
        return hipSuccess;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n16 + 255) / 256, 256);
    hipLaunchKernelGGL(small_upload_kernel, dim3(blocks), dim3(256), 0, stream, pc);
    return hipGetLastError();
}

/* one workgroup: the dense CSR offsets of up to three count arrays, stored in
 * HBM (the gather's) and in mapped host memory (the caller's), plus the plan
 * status word, the window total and the best calls */
__global__ __launch_bounds__(256) void small_collect_kernel(Counts3 cnt, uint32_t n, Offsets3 off, Offsets3 off_host,
                                                            const uint32_t *__restrict__ status,
                                                            const uint64_t *__restrict__ wbase,
                                                            const kgx_best_call *__restrict__ best,
                                                            kgx_best_call *__restrict__ best_host,
                                                            uint32_t *__restrict__ status_host,
                                                            uint64_t *__restrict__ nwin_host)
{
    __shared__ uint64_t lds4[3][4];
    uint64_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base <= n; base += CS_TILE) {
        const uint32_t i0 = base + threadIdx.x * CS_PER;
        for (int a = 0; a < 3; a++) {
            uint64_t tot;
            const uint64_t mine = thread_count(cnt.c[a], n, i0);
            uint64_t at = carry[a] + block_scan(mine, lds4[a], tot) - mine;
            for (uint32_t k = 0; k < CS_PER && i0 + k <= n; k++) {
                off.o[a][i0 + k] = at;
                off_host.o[a][i0 + k] = at;
                if (cnt.c[a] && i0 + k < n)
                    at += cnt.c[a][i0 + k];
            }
            carry[a] += tot;
        }
        __syncthreads(); /* lds4 is rewritten by the next round */
    }
    if (best_host)
        for (uint32_t s = threadIdx.x; s < n; s += blockDim.x)
            best_host[s] = best[s];
    if (threadIdx.x == 0) {
        status_host[0] = status[0];
        nwin_host[0] = wbase[n];
    }
}

hipError_t launch_small_collect(uint32_t n, const uint32_t *c0, const uint32_t *c1, const uint32_t *c2, uint64_t *o0,
                                uint64_t *o1, uint64_t *o2, uint64_t *h0, uint64_t *h1, uint64_t *h2,
                                const uint32_t *status, const uint64_t *wbase, const kgx_best_call *best,
                                kgx_best_call *best_host, uint32_t *status_host, uint64_t *nwin_host,
                                hipStream_t stream)
{
    Counts3 cnt = {{c0, c1, c2}};
    Offsets3 off = {{o0, o1, o2}};
    Offsets3 off_host = {{h0, h1, h2}};
    hipLaunchKernelGGL(small_collect_kernel, dim3(1), dim3(256), 0, stream, cnt, n, off, off_host, status, wbase,
                       best, best_host, status_host, nwin_host);
    return hipGetLastError();
}

/* small_collect + best_call_kernel in one launch for batches of up to
 * SMALL_COLLECT_BEST_SEQ sequences: block b owns offsets [256 b, 256 b + 256)
 * (the last one offset n too), sums the counts before its range itself (at
 * most 3 x 8,192 values from L2), scans its own, and decides its sequences'
 * best calls (best_call_decide, into the device array and the mapped host
 * one).  One launch instead of two, and no one-workgroup serial scan. */
__global__ __launch_bounds__(256) void small_collect_best_kernel(
    Counts3 cnt, uint32_t n, Offsets3 off, Offsets3 off_host, const uint32_t *__restrict__ status,
    const uint64_t *__restrict__ wbase, const kgx_call *__restrict__ calls, const uint32_t *__restrict__ call_count,
    kgx_call *__restrict__ ws, kgx_best_call *__restrict__ best, kgx_best_call *__restrict__ best_host,
    uint32_t *__restrict__ status_host, uint64_t *__restrict__ nwin_host)
{
    __shared__ uint64_t lds_pre[3][4], lds_own[3][4];
    const uint32_t t = threadIdx.x, s0 = blockIdx.x * 256u, i = s0 + t;
    for (int a = 0; a < 3; a++) {
        uint64_t v = 0, before = 0, tot = 0;
        if (cnt.c[a]) {
#pragma unroll 8
            for (uint32_t j = t; j < s0; j += 256)
                v += cnt.c[a][j];
        }
        (void)block_scan(v, lds_pre[a], before);
        const uint64_t mine = cnt.c[a] && i < n ? cnt.c[a][i] : 0;
        const uint64_t at = before + block_scan(mine, lds_own[a], tot) - mine;
        if (i <= n) {
            off.o[a][i] = at;
            off_host.o[a][i] = at;
        }
    }
    if (i < n) {
        const uint64_t w = wbase[i];
        const kgx_best_call b = best_call_decide(calls + w, call_count[i], ws + w);
        best[i] = b;
        if (best_host)
            best_host[i] = b;
    }
    if (blockIdx.x == 0 && t == 0) {
        status_host[0] = status[0];
        nwin_host[0] = wbase[n];
    }
}

hipError_t launch_small_collect_best(uint32_t n, const uint32_t *c0, const uint32_t *c1, const uint32_t *c2,
                                     uint64_t *o0, uint64_t *o1, uint64_t *o2, uint64_t *h0, uint64_t *h1,
                                     uint64_t *h2, const uint32_t *status, const uint64_t *wbase,
                                     const kgx_call *calls, const uint32_t *call_count, kgx_call *ws,
                                     kgx_best_call *best, kgx_best_call *best_host, uint32_t *status_host,
                                     uint64_t *nwin_host, hipStream_t stream)
{
    if (n > SMALL_COLLECT_BEST_SEQ)
        return hipErrorInvalidValue;
    Counts3 cnt = {{c0, c1, c2}};
    Offsets3 off = {{o0, o1, o2}};
    Offsets3 off_host = {{h0, h1, h2}};
    hipLaunchKernelGGL(small_collect_best_kernel, dim3(n / 256 + 1), dim3(256), 0, stream, cnt, n, off, off_host,
                       status, wbase, calls, call_count, ws, best, best_host, status_host, nwin_host);
    return hipGetLastError();
}

/* min(*count, cap) elements of elem_bytes each, src -> dst: the size comes
 * from the device (a chunk's scanned total), the room from the host.  The
 * bytes move as 16-B stores (one 1-KB run per wave instruction over PCIe),
 * the last < 16 as 4-B stores; both ends 16-B aligned. */
__global__ __launch_bounds__(256) void copy_counted_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src,
                                                           const uint64_t *__restrict__ count, uint64_t cap,
                                                           uint32_t elem_bytes)
{
    const uint64_t bytes = (*count < cap ? *count : cap) * elem_bytes;
    const uint64_t n16 = bytes / 16;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = tid; i < n16; i += stride)
        dst[i] = src[i];
    const uint32_t tail = (uint32_t)(bytes - 16 * n16) / 4; /* elem_bytes is a multiple of 4 */
    if (tid < tail)
        reinterpret_cast<uint32_t *>(dst + n16)[tid] = reinterpret_cast<const uint32_t *>(src + n16)[tid];
}

hipError_t launch_copy_counted(void *dst, const void *src, const uint64_t *count, uint64_t cap,
                               uint32_t elem_bytes, int blocks, hipStream_t stream)
{
    if (cap == 0)
        return hipSuccess;
    if (elem_bytes % 4 != 0 || (uintptr_t)dst % 16 != 0 || (uintptr_t)src % 16 != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(copy_counted_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<uint4 *>(dst),
                       static_cast<const uint4 *>(src), count, cap, elem_bytes);
    return hipGetLastError();
}

/* any NUL among bytes [skip, n) of d -> *flag = 1 (a store into mapped host
 * memory).  Residues the device reads straight from the caller's pinned
 * buffer are not NUL-cut on the host (gather_hits' strlen bound, kguts.cc:792),
 * so the host path checks them here and reruns a batch that has one. */
__global__ __launch_bounds__(256) void nul_scan_kernel(const uint4 *__restrict__ d, uint64_t skip, uint64_t n,
                                                       uint32_t *flag)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t n16 = n / 16;
    bool nul = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint4 v = d[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        if (16 * i >= skip) {
            for (int j = 0; j < 4; j++)
                nul |= ((w[j] - 0x01010101u) & ~w[j] & 0x80808080u) != 0;
        } else { /* the first word: bytes before skip are not the batch's */
            for (int b = 0; b < 16; b++)
                nul |= 16 * i + b >= skip && ((w[b / 4] >> (8 * (b % 4))) & 0xFFu) == 0;
        }
    }
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid < n - 16 * n16 && 16 * n16 + tid >= skip)
        nul |= reinterpret_cast<const uint8_t *>(d)[16 * n16 + tid] == 0;
    if (__ballot(nul) && lane_id() == 0)
        __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_nul_scan(const uint8_t *d, uint64_t skip, uint64_t n, uint32_t *flag_mapped, hipStream_t stream)
{
    if (n <= skip)
        return hipSuccess;
    if ((uintptr_t)d % 16 != 0)
        return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n / 16 + 255) / 256 + 1, 1024);
    hipLaunchKernelGGL(nul_scan_kernel, dim3(blocks), dim3(256), 0, stream, reinterpret_cast<const uint4 *>(d), skip,
                       n, flag_mapped);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* copy to mapped pinned host memory: the device's own stores stream the     */
/* results over PCIe (one contiguous 1-KB run per wave instruction), so the */
/* D2H needs no DMA-engine slot and overlaps other streams' H2D copies      */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(256) void copy16_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src,
                                                     uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = src[i];
}

__global__ __launch_bounds__(256) void copy4_kernel(uint32_t *__restrict__ dst, const uint32_t *__restrict__ src,
                                                    uint64_t n)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = src[i];
}

hipError_t launch_copy_to_host(void *dst, const void *src, uint64_t bytes, int copy_blocks, hipStream_t stream)
{
    if (bytes == 0)
        return hipSuccess;
    const bool v16 = ((uintptr_t)dst % 16 == 0) && ((uintptr_t)src % 16 == 0) && bytes % 16 == 0;
    if (!v16 && (((uintptr_t)dst | (uintptr_t)src | bytes) % 4 != 0))
        return hipErrorInvalidValue;
    const uint64_t n = v16 ? bytes / 16 : bytes / 4;
    /* PCIe writes are posted: a few waves keep the link busy, and a full
     * grid would starve the kernels of the other stream (latency-bound
     * scorer, plan) that this copy is meant to run beside */
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)copy_blocks);
    if (v16)
        hipLaunchKernelGGL(copy16_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<uint4 *>(dst),
                           static_cast<const uint4 *>(src), n);
    else
        hipLaunchKernelGGL(copy4_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<uint32_t *>(dst),
                           static_cast<const uint32_t *>(src), n);
    return hipGetLastError();
}

/* several spans in one launch (blockIdx.y = span): a collect's counts, totals
 * and best calls cost one kernel instead of five back-to-back ones */
__global__ __launch_bounds__(256) void copy_spans_kernel(CopySpans sp)
{
    const uint32_t k = blockIdx.y;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t i0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (sp.v16[k]) {
        uint4 *d = static_cast<uint4 *>(sp.dst[k]);
        const uint4 *s = static_cast<const uint4 *>(sp.src[k]);
        for (uint64_t i = i0; i < sp.n[k]; i += stride)
            d[i] = s[i];
    } else {
        uint32_t *d = static_cast<uint32_t *>(sp.dst[k]);
        const uint32_t *s = static_cast<const uint32_t *>(sp.src[k]);
        for (uint64_t i = i0; i < sp.n[k]; i += stride)
            d[i] = s[i];
    }
}

hipError_t launch_copy_spans(CopySpans sp, int copy_blocks, hipStream_t stream)
{
    if (sp.count == 0)
        return hipSuccess;
    if (sp.count > CopySpans::kMax)
        return hipErrorInvalidValue;
    uint64_t most = 1;
    for (int k = 0; k < sp.count; k++) {
        const uintptr_t d = reinterpret_cast<uintptr_t>(sp.dst[k]), s = reinterpret_cast<uintptr_t>(sp.src[k]);
        const uint64_t bytes = sp.n[k];
        sp.v16[k] = d % 16 == 0 && s % 16 == 0 && bytes % 16 == 0;
        if (!sp.v16[k] && ((d | s | bytes) % 4 != 0))
            return hipErrorInvalidValue;
        sp.n[k] = sp.v16[k] ? bytes / 16 : bytes / 4;
        most = std::max(most, sp.n[k]);
    }
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((most + 255) / 256, (uint64_t)copy_blocks);
    hipLaunchKernelGGL(copy_spans_kernel, dim3(blocks, (uint32_t)sp.count), dim3(256), 0, stream, sp);
    return hipGetLastError();
}

}  // namespace kgx
