/*
 * kgx_inflate.hip -- blocked gzip (BGZF) members inflated on the device.
 *
 * inflate_members_kernel: one wave per member, four waves per workgroup.  A
 * member's compressed bytes and its output slot come from the member table
 * the host's framing walk made (kgx_gz_member; out_off is the exclusive scan
 * of the ISIZEs).  The decoder is kgx_inflate.h's inflate_raw, the code the
 * host runs, under the WaveIO policy below:
 *
 *  - the symbol decode is wave-uniform: every lane holds the same bit buffer
 *    and position and takes the same branches, so the input reads are uniform
 *    loads and no lane waits for another; what comes back from memory is
 *    declared uniform (uni(): v_readfirstlane), so the bit buffer, the
 *    pointers and the branches are scalar;
 *  - the code tables (InflateTables, 3.6 KB) are in the wave's own LDS; their
 *    primary tables are filled by the lanes together;
 *  - the lanes move the bytes.  Literals gather in a register per lane, 64 to
 *    a store.  A match of L bytes at distance D is stored by lane i taking
 *    source byte i (D >= L) or i mod D (D < L: a run, D = 1 being a run of
 *    one quality character), 64 bytes to a pass; a stored block is copied the
 *    same way.
 *
 * Ordering.  A match loads bytes that other lanes of the same wave stored a
 * few instructions earlier (the previous match, or the literals just
 * flushed), to global memory.  The rule used: a wave's vector memory
 * instructions go to its CU's vector L1 in issue order, and that L1 serves
 * every lane of the wave, so a load issued after a store to the same address
 * returns the stored byte whichever lane stored it -- the AMDGPU memory
 * model's wavefront scope, at which a fence needs no cache action and no
 * wait.  What remains is the compiler: match() and stored() put a
 * wavefront-scope release-acquire fence between the earlier stores and the
 * loads, so neither is moved across the other.  Inside one match the source
 * bytes all lie before the match's first byte, so its own passes do not
 * depend on one another.  A window in LDS was not needed for this and would
 * cost occupancy (32 KiB a wave).
 *
 * Safety.  Every bound of inflate_raw holds here as on the host: nothing is
 * read outside the member's [in_off, in_off + in_len) and nothing stored
 * outside its [out_off, out_off + out_len).  A failing member writes its
 * reason and bit position to status[m] and its wave leaves.
 *
 * CRC.  After the last block each lane runs the bytewise table CRC over its
 * contiguous 1/64 of the output (the 1-KiB table in LDS, built in the
 * prologue), the first lane from 0xffffffff and the others from 0, and the
 * registers are joined by multiplying each with x^(8 * bytes after its slice)
 * modulo the CRC polynomial (kgx_inflate.h, crc32_xpow8) and XOR over the
 * wave.  The lanes load what the wave stored: the same ordering rule.
 *
 * Statistics go to stats[m], one record per member, summed on the host.  No
 * atomics, no scratch; every store is an ordinary vector store.
 */
#include "kgx_device.h"
#include "kgx_inflate.h"
#include "kgx_rt.h"

using namespace kgx;

namespace {

constexpr uint32_t INFLATE_WAVES = 4;

__device__ __forceinline__ void wave_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct WaveIO {
    uint32_t lane_;
    uint32_t pending;  /* literals gathered, 0..63; wave-uniform */
    uint8_t *pend_at;  /* where the first of them goes */
    uint32_t mine;     /* this lane's literal */
    __device__ uint32_t lane() const { return lane_; }
    __device__ uint32_t lanes() const { return 64u; }
    /* LDS tables: written by some lanes, read by all */
    __device__ void sync() const { wave_fence(); }
    __device__ uint32_t uni(uint32_t v) const { return __builtin_amdgcn_readfirstlane(v); }
    __device__ uint64_t uni(uint64_t v) const { return (uint64_t)uni((uint32_t)(v >> 32)) << 32 | uni((uint32_t)v); }
    __device__ void flush()
    {
        if (lane_ < pending)
            pend_at[lane_] = (uint8_t)mine;
        pending = 0;
    }
    __device__ void literal(uint8_t *dst, uint8_t v)
    {
        if (pending == 0)
            pend_at = dst;
        if (lane_ == pending)
            mine = v;
        if (++pending == 64u)
            flush();
    }
    __device__ void match(uint8_t *dst, uint32_t dist, uint32_t len)
    {
        flush();
        wave_fence();
        const uint8_t *src = dst - dist;
        for (uint32_t i = lane_; i < len; i += 64u) {
            const uint32_t k = dist >= len ? i : dist == 1u ? 0u : i % dist;
            dst[i] = src[k];
        }
        wave_fence();
    }
    __device__ void stored(uint8_t *dst, const uint8_t *src, uint32_t len)
    {
        for (uint32_t i = lane_; i < len; i += 64u)
            dst[i] = src[i];
        wave_fence();
    }
};

__global__ __launch_bounds__(64 * INFLATE_WAVES) void inflate_members_kernel(const uint8_t *__restrict__ gz,
                                                                             const kgx_gz_member *__restrict__ members,
                                                                             uint32_t n_members, uint8_t *out,
                                                                             kgx_gz_status *__restrict__ status,
                                                                             kgx_inflate_stats *__restrict__ stats)
{
    __shared__ InflateTables tables[INFLATE_WAVES];
    __shared__ uint32_t crc_table[256];
    crc_table[threadIdx.x] = crc32_table_entry(threadIdx.x);
    __syncthreads();
    /* the wave's number is the same in its lanes: say so, and the member's record, its
     * pointers and the whole decode state stay in scalar registers */
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t m = blockIdx.x * INFLATE_WAVES + wave;
    if (m >= n_members)
        return;
    const kgx_gz_member mb = members[m];
    const uint8_t *in = gz + mb.in_off;
    uint8_t *o = out + mb.out_off;
    WaveIO io{lane, 0u, o, 0u};
    InflateStats st;
    InflateResult r = inflate_raw(in, in + mb.in_len, o, o + mb.out_len, &tables[wave], &st, io);
    if (r.reason == INF_OK && r.out_len != mb.out_len)
        r.reason = INF_OUTPUT_SHORT;
    if (r.reason == INF_OK) {
        wave_fence();
        const uint32_t n = mb.out_len, slice = (n + 63u) / 64u;
        const uint32_t a = min(lane * slice, n), b = min(a + slice, n);
        uint32_t reg = crc32_run(crc_table, lane == 0 ? 0xffffffffu : 0u, o + a, b - a);
        reg = crc32_mulmod(reg, crc32_xpow8(n - b));
        for (uint32_t d = 32; d; d >>= 1)
            reg ^= (uint32_t)__shfl_xor((int)reg, (int)d, 64);
        if (~reg != mb.crc)
            r.reason = INF_CRC;
    }
    if (lane == 0) {
        status[m] = kgx_gz_status{r.reason, (uint32_t)r.out_len, r.bit_pos};
        stats[m] = kgx_inflate_stats{st.stored_blocks, st.fixed_blocks, st.dynamic_blocks, st.max_code_len,
                                     st.max_distance,  st.max_length,   st.overlap,        st.matches};
    }
}

}  // namespace

namespace kgx {

hipError_t launch_inflate_members(const uint8_t *gz, const kgx_gz_member *members, uint32_t n_members, uint8_t *out,
                                  kgx_gz_status *status, kgx_inflate_stats *stats, hipStream_t stream)
{
    if (n_members == 0)
        return hipSuccess;
    hipLaunchKernelGGL(inflate_members_kernel, dim3((n_members + INFLATE_WAVES - 1) / INFLATE_WAVES),
                       dim3(64 * INFLATE_WAVES), 0, stream, gz, members, n_members, out, status, stats);
    return hipGetLastError();
}

}  // namespace kgx
