/*
 * kgx_plan.hip -- the plan of a batch, first step of the lookup path
 * (plan -> probe -> score -> gather).
 *
 *   plan   : wbase = exclusive scan of windows per sequence; tile -> first
 *            sequence map (two launches, 1,024 sequences per workgroup; one
 *            launch with a look-back; one workgroup for small batches)
 */
#include "kgx_device.h"

namespace kgx {

constexpr uint32_t PLAN_PER = 4;               /* sequences per thread */
constexpr uint32_t PLAN_TILE = 256 * PLAN_PER; /* sequences per workgroup */

__device__ __forceinline__ uint64_t thread_windows(const uint64_t *seq_off, uint32_t n, uint32_t s0)
{
    uint64_t w = 0;
    for (uint32_t k = 0; k < PLAN_PER; k++)
        if (s0 + k < n)
            w += windows_of(seq_off[s0 + k + 1] - seq_off[s0 + k]);
    return w;
}

/* the batch's offsets are usable iff they are monotone and span at most
 * n_residues bytes (kgx.h, kgx_run_device); then every window count is
 * bounded by its length and the plan's buffers (sized from n_residues) hold
 * the batch.  Checked per thread over its PLAN_PER sequences. */
__device__ __forceinline__ bool thread_offsets_bad(const uint64_t *seq_off, uint32_t n, uint32_t s0,
                                                   uint64_t n_residues)
{
    const uint64_t first = seq_off[0];
    bool bad = seq_off[n] < first || seq_off[n] - first > n_residues;
    for (uint32_t k = 0; k < PLAN_PER; k++)
        if (s0 + k < n)
            bad |= seq_off[s0 + k + 1] < seq_off[s0 + k];
    return bad;
}

constexpr uint64_t PLAN_BAD = 1ull << 63; /* marks a workgroup sum whose offsets are bad */

/* the longest sequence's windows (capped at 2^32 - 1) of this thread's PLAN_PER */
__device__ __forceinline__ uint32_t thread_max_windows(const uint64_t *seq_off, uint32_t n, uint32_t s0)
{
    uint64_t m = 0;
    for (uint32_t k = 0; k < PLAN_PER; k++)
        if (s0 + k < n)
            m = max(m, windows_of(seq_off[s0 + k + 1] - seq_off[s0 + k]));
    return (uint32_t)min<uint64_t>(m, 0xFFFFFFFFull);
}

__global__ __launch_bounds__(256) void plan_reduce_kernel(const uint64_t *__restrict__ seq_off,
                                                          uint32_t n, uint64_t n_residues,
                                                          uint64_t *__restrict__ sums, uint32_t *__restrict__ maxw)
{
    __shared__ uint64_t lds4[4];
    __shared__ uint32_t lmax[4];
    uint64_t total;
    const uint32_t s0 = blockIdx.x * PLAN_TILE + threadIdx.x * PLAN_PER;
    const bool bad = __syncthreads_or(thread_offsets_bad(seq_off, n, s0, n_residues));
    block_scan(bad ? 0 : thread_windows(seq_off, n, s0), lds4, total);
    /* the workgroup's longest sequence (scorer dispatch, plan_sums_scan) */
    uint32_t m = bad ? 0u : thread_max_windows(seq_off, n, s0);
    for (uint32_t off = 32; off; off >>= 1)
        m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if ((threadIdx.x & 63u) == 0)
        lmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        sums[blockIdx.x] = bad ? PLAN_BAD : total;
        maxw[blockIdx.x] = max(max(lmax[0], lmax[1]), max(lmax[2], lmax[3]));
    }
}

/* exclusive scan of the workgroup sums in place, one workgroup of 1,024
 * threads, each scanning 16 consecutive sums per round (a 9.9M-fragment fq
 * chunk's 9.7k sums: one round).  (Each plan_scan workgroup used to add up
 * all earlier sums itself: quadratic in the number of workgroups, 0.5 ms for
 * the 9.9M fragments of a 1M-read fq chunk; then 256 threads in rounds of
 * 256: 31 us.) */
constexpr uint32_t SUMS_PER = 16;

/* SUMS_THREADS 256 for up to 4,096 sums (C2: 98): a 4-wave workgroup finds a
 * slot beside the other context's probe at once, where a 16-wave one waited
 * for that probe to drain (550 us stretched, kernel trace r2zr; 9 us, r2zs).
 * The 12-14 us between consecutive probes did not change: that is the
 * cross-queue event wait, not the plan. */
template <uint32_t SUMS_THREADS>
__global__ __launch_bounds__(SUMS_THREADS) void plan_sums_scan_kernel(uint64_t *__restrict__ sums, uint32_t groups,
                                                                      const uint32_t *__restrict__ maxw,
                                                                      uint32_t *__restrict__ status)
{
    __shared__ uint64_t wsum[SUMS_THREADS / 64];
    __shared__ uint32_t wmax[SUMS_THREADS / 64];
    /* any workgroup that saw bad offsets empties the whole batch (sums[groups]
     * = 1 tells plan_scan) and raises the context's status word; status[1] =
     * the batch's longest sequence in windows (the scorer's dispatch) */
    bool bad = false;
    uint32_t m = 0;
    for (uint32_t i = threadIdx.x; i < groups; i += SUMS_THREADS) {
        bad |= (sums[i] & PLAN_BAD) != 0;
        m = max(m, maxw[i]);
    }
    for (uint32_t off = 32; off; off >>= 1)
        m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if ((threadIdx.x & 63u) == 0)
        wmax[threadIdx.x >> 6] = m;
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        uint32_t mm = 0;
        for (uint32_t w = 0; w < SUMS_THREADS / 64; w++)
            mm = max(mm, wmax[w]);
        status[1] = bad ? 0u : mm;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < groups; base += SUMS_THREADS * SUMS_PER) {
        const uint32_t i0 = base + threadIdx.x * SUMS_PER;
        uint64_t v[SUMS_PER], t = 0;
#pragma unroll
        for (uint32_t k = 0; k < SUMS_PER; k++) {
            v[k] = i0 + k < groups && !bad ? sums[i0 + k] : 0;
            t += v[k];
        }
        /* exclusive prefix of the threads' totals: wave scan, then the waves' sums */
        uint64_t x = t;
        for (uint32_t off = 1; off < 64; off <<= 1) {
            const uint64_t y = __shfl_up(x, off);
            if (lane >= off)
                x += y;
        }
        if (lane == 63)
            wsum[wave] = x;
        __syncthreads();
        uint64_t pre = carry, tot = 0;
        for (uint32_t w = 0; w < SUMS_THREADS / 64; w++) {
            if (w < wave)
                pre += wsum[w];
            tot += wsum[w];
        }
        pre += x - t;
#pragma unroll
        for (uint32_t k = 0; k < SUMS_PER; k++) {
            if (i0 + k < groups)
                sums[i0 + k] = pre;
            pre += v[k];
        }
        carry += tot;
        __syncthreads(); /* wsum is rewritten by the next round */
    }
    if (threadIdx.x == 0) {
        sums[groups] = bad ? 1 : 0;
        status[0] = bad ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void plan_scan_kernel(const uint64_t *__restrict__ seq_off,
                                                        uint32_t n, const uint64_t *__restrict__ sums,
                                                        uint64_t *__restrict__ wbase,
                                                        uint32_t *__restrict__ tile_seq,
                                                        uint32_t tile_windows)
{
    __shared__ uint64_t lds_b[4];
    const uint64_t before = sums[blockIdx.x]; /* windows of all earlier workgroups */
    const bool bad = sums[gridDim.x] != 0;    /* bad offsets: an empty batch */

    const uint32_t s0 = blockIdx.x * PLAN_TILE + threadIdx.x * PLAN_PER;
    const uint64_t mine = bad ? 0 : thread_windows(seq_off, n, s0);
    uint64_t tot;
    const uint64_t incl = block_scan(mine, lds_b, tot);
    uint64_t wb = before + incl - mine;
    for (uint32_t k = 0; k < PLAN_PER; k++) {
        const uint32_t s = s0 + k;
        if (s >= n)
            break;
        const uint64_t we = wb + (bad ? 0 : windows_of(seq_off[s + 1] - seq_off[s]));
        wbase[s] = wb;
        /* tiles whose first window lies in [wb, we) start inside sequence s */
        for (uint64_t t = (wb + tile_windows - 1) / tile_windows; t * tile_windows < we; t++)
            tile_seq[t] = s;
        wb = we;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255)
        wbase[n] = before + tot;
}

/*
 * The plan in ONE launch (the default; KGX_PLAN_FUSED=0: the three kernels
 * above): plan_reduce, plan_sums_scan and plan_scan fused by a decoupled
 * look-back over the workgroups of PLAN_TILE sequences, as fq_anchor_fused
 * does for fragments.  Workgroup g publishes its windows (state 1) and, once
 * it has summed the states of the workgroups before it -- 64 at a time, one
 * per lane of wave 0, until one holds an inclusive prefix (state 2) -- its own
 * inclusive prefix; then it writes its sequences' window bases and tile
 * owners exactly as plan_scan.  Workgroups start in index order, so every
 * state waited on belongs to a workgroup already running.  State words are
 * state << 62 | value, relaxed device-scope atomics; after them in `look`: the
 * finished-workgroup ticket, the bad-offsets flag and the longest sequence.
 * The workgroup that finishes last writes the status words, empties the
 * batch when any workgroup saw bad offsets (every window base 0: what the
 * three kernels give), and zeroes `look` for the next launch (zero-filled
 * when allocated).  Tile owners are written only below max_tiles: with bad
 * offsets a workgroup's prefix may pass the buffer before the batch is
 * emptied.
 */
constexpr uint64_t LOOK_MASK = (1ull << 62) - 1;

__global__ __launch_bounds__(256) void plan_fused_kernel(const uint64_t *__restrict__ seq_off, uint32_t n,
                                                         uint64_t n_residues, uint64_t *__restrict__ wbase,
                                                         uint32_t *__restrict__ tile_seq, uint32_t tile_windows,
                                                         uint64_t max_tiles, uint64_t *__restrict__ look,
                                                         uint32_t groups, uint32_t *__restrict__ status)
{
    __shared__ uint64_t lds4[4];
    __shared__ uint32_t lmax[4];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_last;
    uint32_t *ctl = reinterpret_cast<uint32_t *>(look + groups); /* ticket, bad, longest */
    const uint32_t g = blockIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s0 = g * PLAN_TILE + threadIdx.x * PLAN_PER;
    const bool bad = __syncthreads_or(thread_offsets_bad(seq_off, n, s0, n_residues));
    const uint64_t mine = bad ? 0 : thread_windows(seq_off, n, s0);
    uint64_t tot;
    const uint64_t incl = block_scan(mine, lds4, tot);
    uint32_t m = bad ? 0u : thread_max_windows(seq_off, n, s0);
    for (uint32_t off = 32; off; off >>= 1)
        m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if (lane == 0)
        lmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x < 64) {
        if (threadIdx.x == 0) {
            if (bad)
                __hip_atomic_fetch_or(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&ctl[2], max(max(lmax[0], lmax[1]), max(lmax[2], lmax[3])), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&look[g], (g == 0 ? 2ull : 1ull) << 62 | tot, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        /* look back: lane l examines workgroup j - l */
        uint64_t x = 0;
        for (int64_t j = (int64_t)g - 1; j >= 0; j -= 64) {
            const int64_t idx = j - (int64_t)lane;
            uint64_t v = 2ull << 62; /* before workgroup 0: a zero prefix */
            if (idx >= 0)
                do {
                    v = __hip_atomic_load(&look[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } while ((v >> 62) == 0);
            const uint64_t pm = __ballot((v >> 62) == 2);
            const uint32_t upto = pm ? (uint32_t)__builtin_ctzll(pm) : 63u; /* lanes 0..upto count */
            uint64_t y = lane <= upto ? v & LOOK_MASK : 0;
            for (uint32_t o = 32; o; o >>= 1)
                y += __shfl_xor(y, (int)o);
            x += y;
            if (pm)
                break;
        }
        if (threadIdx.x == 0) {
            if (g)
                __hip_atomic_store(&look[g], 2ull << 62 | ((x + tot) & LOOK_MASK), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            s_prefix = x;
        }
    }
    __syncthreads();
    const uint64_t before = s_prefix;
    uint64_t wb = before + incl - mine;
    for (uint32_t k = 0; k < PLAN_PER; k++) {
        const uint32_t s = s0 + k;
        if (s >= n)
            break;
        const uint64_t we = wb + (bad ? 0 : windows_of(seq_off[s + 1] - seq_off[s]));
        wbase[s] = wb;
        /* tiles whose first window lies in [wb, we) start inside sequence s */
        for (uint64_t t = (wb + tile_windows - 1) / tile_windows; t * tile_windows < we && t < max_tiles; t++)
            tile_seq[t] = s;
        wb = we;
    }
    if (g == groups - 1 && threadIdx.x == 255)
        wbase[n] = before + tot;
    /* the last workgroup to finish: status, the bad-offsets fix-up, the reset */
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&ctl[0], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
    __syncthreads();
    if (!s_last)
        return;
    __threadfence();
    const uint32_t any_bad = __hip_atomic_load(&ctl[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (any_bad)
        for (uint64_t s = threadIdx.x; s <= n; s += 256)
            wbase[s] = 0;
    if (threadIdx.x == 0) {
        status[0] = any_bad ? 1u : 0u;
        status[1] = any_bad ? 0u : __hip_atomic_load(&ctl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (uint32_t j = threadIdx.x; j < groups; j += 256)
        __hip_atomic_store(&look[j], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x < 3)
        __hip_atomic_store(&ctl[threadIdx.x], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* The plan of a batch of up to PLAN_ONE_MAX sequences in ONE workgroup of
 * 1,024 threads (option plan_fused 2): thread t takes a contiguous run of
 * sequences, the runs' window counts are scanned across the workgroup, and
 * each thread writes its sequences' window bases and tile owners -- one
 * launch, nothing to wait on, one CU beside the probe.  Bad offsets empty the
 * batch as the three kernels do. */
constexpr uint32_t PLAN_ONE_MAX = 1u << 18;

__global__ __launch_bounds__(1024) void plan_one_kernel(const uint64_t *__restrict__ seq_off, uint32_t n,
                                                        uint64_t n_residues, uint64_t *__restrict__ wbase,
                                                        uint32_t *__restrict__ tile_seq, uint32_t tile_windows,
                                                        uint64_t max_tiles, uint32_t *__restrict__ status)
{
    __shared__ uint64_t wsum[16];
    __shared__ uint32_t wmax[16];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint32_t per = (n + 1023) / 1024;
    const uint32_t s0 = min(n, t * per), s1 = min(n, s0 + per);
    const uint64_t first = seq_off[0], last = seq_off[n];
    bool bad = last < first || last - first > n_residues;
    uint64_t w = 0;
    uint32_t m = 0;
    for (uint32_t s = s0; s < s1; s++) {
        const uint64_t a = seq_off[s], b = seq_off[s + 1];
        bad |= b < a;
        const uint64_t ww = b >= a ? windows_of(b - a) : 0;
        w += ww;
        m = max(m, (uint32_t)min<uint64_t>(ww, 0xFFFFFFFFull));
    }
    bad = __syncthreads_or(bad);
    /* exclusive scan of the threads' windows: waves, then the 16 wave sums */
    uint64_t x = w;
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint64_t y = __shfl_up(x, off);
        if (lane >= off)
            x += y;
    }
    for (uint32_t off = 32; off; off >>= 1)
        m = max(m, (uint32_t)__shfl_xor((int)m, (int)off));
    if (lane == 63)
        wsum[wave] = x;
    if (lane == 0)
        wmax[wave] = m;
    __syncthreads();
    uint64_t before = 0, total = 0;
    uint32_t mm = 0;
    for (uint32_t i = 0; i < 16; i++) {
        before += i < wave ? wsum[i] : 0;
        total += wsum[i];
        mm = max(mm, wmax[i]);
    }
    uint64_t wb = bad ? 0 : before + x - w;
    for (uint32_t s = s0; s < s1; s++) {
        const uint64_t we = wb + (bad ? 0 : windows_of(seq_off[s + 1] - seq_off[s]));
        wbase[s] = wb;
        for (uint64_t k = (wb + tile_windows - 1) / tile_windows; k * tile_windows < we && k < max_tiles; k++)
            tile_seq[k] = s;
        wb = we;
    }
    if (t == 0) {
        wbase[n] = bad ? 0 : total;
        status[0] = bad ? 1u : 0u;
        status[1] = bad ? 0u : mm;
    }
}

hipError_t launch_plan_one(const uint64_t *seq_off, uint32_t n_seq, uint64_t n_residues, uint64_t *wbase,
                           uint32_t *tile_seq, uint32_t tile_windows, uint64_t max_tiles, uint32_t *status,
                           hipStream_t stream)
{
    if (n_seq > PLAN_ONE_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(plan_one_kernel, dim3(1), dim3(1024), 0, stream, seq_off, n_seq, n_residues, wbase, tile_seq,
                       tile_windows, max_tiles, status);
    return hipGetLastError();
}

size_t plan_look_bytes(uint32_t n_seq) { return ((size_t)n_seq / PLAN_TILE + 1) * sizeof(uint64_t) + 16; }

hipError_t launch_plan_fused(const uint64_t *seq_off, uint32_t n_seq, uint64_t n_residues, uint64_t *wbase,
                             uint32_t *tile_seq, uint32_t tile_windows, uint64_t max_tiles, void *look,
                             uint32_t *status, hipStream_t stream)
{
    const uint32_t groups = n_seq / PLAN_TILE + 1; /* >= 1 so wbase[n] is written */
    hipLaunchKernelGGL(plan_fused_kernel, dim3(groups), dim3(256), 0, stream, seq_off, n_seq, n_residues, wbase,
                       tile_seq, tile_windows, max_tiles, static_cast<uint64_t *>(look), groups, status);
    return hipGetLastError();
}

/* the workgroup sums + the bad-offsets word, then the workgroups' longest sequences */
size_t plan_workspace_bytes(uint32_t n_seq)
{
    return ((size_t)n_seq / PLAN_TILE + 2) * (sizeof(uint64_t) + sizeof(uint32_t));
}

hipError_t launch_plan(const uint64_t *seq_off, uint32_t n_seq, uint64_t n_residues, uint64_t *wbase,
                       uint32_t *tile_seq, uint32_t tile_windows, void *workspace, uint32_t *status,
                       hipStream_t stream)
{
    const uint32_t groups = n_seq / PLAN_TILE + 1; /* >= 1 so wbase[n] is written */
    uint32_t *maxw = reinterpret_cast<uint32_t *>(static_cast<uint64_t *>(workspace) + groups + 2);
    hipLaunchKernelGGL(plan_reduce_kernel, dim3(groups), dim3(256), 0, stream, seq_off, n_seq, n_residues,
                       static_cast<uint64_t *>(workspace), maxw);
    if (groups <= 256 * SUMS_PER)
        hipLaunchKernelGGL(plan_sums_scan_kernel<256>, dim3(1), dim3(256), 0, stream,
                           static_cast<uint64_t *>(workspace), groups, maxw, status);
    else
        hipLaunchKernelGGL(plan_sums_scan_kernel<1024>, dim3(1), dim3(1024), 0, stream,
                           static_cast<uint64_t *>(workspace), groups, maxw, status);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(groups), dim3(256), 0, stream, seq_off, n_seq,
                       static_cast<const uint64_t *>(workspace), wbase, tile_seq, tile_windows);
    return hipGetLastError();
}

}  // namespace kgx
