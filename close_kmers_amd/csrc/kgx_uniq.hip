/*
 * kgx_uniq.hip -- unique_prots.cc on the device: proteins
 * grouped by the set of signature k-mers the image hits in them.
 *
 * The reference (unique_prots.cc:61-109) collects hit.which_kmer per protein
 * through hit_cb -- every window lookup_hash_entry finds, before the gap rule,
 * the order constraint, the hit cap and min_hits -- into a std::set, and
 * prints a std::map<std::set<u64>, std::vector<std::string>>.  Here the corpus
 * runs in pieces of whole sequences through the context's plan and probe (no
 * scorer); per piece
 *   - one kernel turns the tiled hits into `sequence << 35 | key` words,
 *   - a radix sort over the bits in use and a unique leave each sequence's
 *     ascending key list, appended to the corpus' key buffer;
 * then, over the whole corpus,
 *   - (size, digest) per sequence: a thread per short list, a wave per long,
 *   - a merge sort of the sequence indices by (digest, size, list, index),
 *   - the exact head test: a wave per sorted sequence compares its list with
 *     its predecessor's, whatever the digests say,
 *   - a merge sort of the group heads by list alone, the std::map order,
 *   - the gathers into the group CSR, group_of and the groups' key lists.
 * No hit and no per-sequence list reaches the host.
 */
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "kgx.h"
#include "kgx_device.h"
#include "kgx_rt.h"
#include "kgx_tiled.h"

namespace kgx {

constexpr uint64_t kUniqPiece = 1ull << 25;      /* piece_residues 0 */
constexpr uint32_t kUniqPieceSeqs = 1u << 29;    /* a pair word has 64 - 35 bits of sequence */
constexpr uint32_t kUniqKeyBits = 35;            /* 20^8 < 2^35 */
constexpr uint64_t kUniqKeyMask = (1ull << kUniqKeyBits) - 1;
/* the digest of a list of at most this many keys is one thread's loop, of a
 * longer one a wave's (tests/test_gpu_unique.py names it) */
constexpr uint32_t kUniqThreadList = 32;
/* keys per step of the head test and of the list gather: one per lane */
constexpr uint32_t kUniqWaveStep = 64;

/* ---- pairs ---- */

__global__ __launch_bounds__(256) void uniq_tile_counts_kernel(Tiled t, uint64_t n_tiles, uint32_t *counts)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tiles)
        counts[i] = tile_count(t, i);
    else if (i == n_tiles)
        counts[i] = 0;
}

/* one word per hit, compacted by the tiles' bases: sequence << 35 | key */
__global__ __launch_bounds__(256) void uniq_pairs_kernel(Tiled t, uint64_t n_tiles, const uint32_t *__restrict__ tile_base,
                                                         uint64_t *__restrict__ pairs)
{
    const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t tile = slot / t.T;
    const uint32_t i = (uint32_t)(slot % t.T);
    if (tile >= n_tiles || i >= tile_base[tile + 1] - tile_base[tile])
        return;
    uint64_t key;
    uint32_t seq;
    hit_key_seq(t, tile, i, key, seq);
    pairs[tile_base[tile] + i] = (uint64_t)seq << kUniqKeyBits | (key & kUniqKeyMask);
}

/* ---- sets ---- */

/* uq[0, n_u): a piece's sorted distinct pair words.  Sequence j of the piece
 * starts at the first word not below j << 35; set_off is the run's array at the
 * piece's first sequence and takes m + 1 entries (the last is the next
 * piece's first, or the corpus' total) */
__global__ __launch_bounds__(256) void uniq_set_off_kernel(const uint64_t *__restrict__ uq, uint64_t n_u, uint32_t m,
                                                           uint64_t k0, uint64_t *__restrict__ set_off)
{
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m)
        return;
    uint64_t lo = 0, hi = n_u;
    if (j == m)
        lo = n_u;
    else {
        const uint64_t want = j << kUniqKeyBits;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (uq[mid] < want)
                lo = mid + 1;
            else
                hi = mid;
        }
    }
    set_off[j] = k0 + lo;
}

__global__ __launch_bounds__(256) void uniq_strip_kernel(const uint64_t *__restrict__ uq, uint64_t n_u,
                                                         uint64_t *__restrict__ keys)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_u)
        keys[i] = uq[i] & kUniqKeyMask;
}

/* ---- the corpus' lists ---- */

struct UniqLists {
    const uint64_t *set_off; /* n + 1 */
    const uint64_t *keys;
    const uint64_t *digest; /* n, masked */
    uint32_t n;
};

/* a list's digest: the sum of a mixer over its keys, so lanes may take the
 * keys in any split and add their parts */
__device__ __forceinline__ uint64_t uniq_mix(uint64_t key) { return mix64(key); }

__global__ __launch_bounds__(256) void uniq_digest_thread_kernel(const uint64_t *__restrict__ set_off,
                                                                 const uint64_t *__restrict__ keys, uint32_t n,
                                                                 uint64_t mask, uint64_t *__restrict__ digest)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const uint64_t a = set_off[i], b = set_off[i + 1];
    if (b - a > kUniqThreadList)
        return;
    uint64_t d = 0;
    for (uint64_t k = a; k < b; k++)
        d += uniq_mix(keys[k]);
    digest[i] = d & mask;
}

__global__ __launch_bounds__(256) void uniq_digest_wave_kernel(const uint64_t *__restrict__ set_off,
                                                               const uint64_t *__restrict__ keys, uint32_t n,
                                                               uint64_t mask, uint64_t *__restrict__ digest)
{
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (i >= n)
        return;
    const uint64_t a = set_off[i], b = set_off[i + 1];
    if (b - a <= kUniqThreadList)
        return;
    uint64_t d = 0;
    for (uint64_t k = a + lane_id(); k < b; k += 64)
        d += uniq_mix(keys[k]);
    for (int off = 32; off; off >>= 1)
        d += __shfl_xor(d, off);
    if (lane_id() == 0)
        digest[i] = d & mask;
}

/* lists a and b compared as std::set<u64> compares: key by key (all 64 bits
 * of a key), a proper prefix first */
__host__ __device__ inline int uniq_list_cmp(const UniqLists &v, uint32_t a, uint32_t b)
{
    const uint64_t oa = v.set_off[a], ob = v.set_off[b];
    const uint64_t la = v.set_off[a + 1] - oa, lb = v.set_off[b + 1] - ob;
    const uint64_t l = la < lb ? la : lb;
    for (uint64_t k = 0; k < l; k++) {
        const uint64_t x = v.keys[oa + k], y = v.keys[ob + k];
        if (x != y)
            return x < y ? -1 : 1;
    }
    return la == lb ? 0 : la < lb ? -1 : 1;
}

/* the grouping order: (digest, size, list, index).  An index that is not
 * below n (a sort's padding) is above every sequence and reads nothing. */
struct UniqGroupLess {
    UniqLists v;
    unsigned long long *walks;
    __host__ __device__ bool operator()(uint32_t a, uint32_t b) const
    {
        if (a >= v.n || b >= v.n)
            return a < b;
        const uint64_t da = v.digest[a], db = v.digest[b];
        if (da != db)
            return da < db;
        const uint64_t la = v.set_off[a + 1] - v.set_off[a], lb = v.set_off[b + 1] - v.set_off[b];
        if (la != lb)
            return la < lb;
        if (la == 0)
            return a < b;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicAdd(walks, 1ull);
#endif
        const int c = uniq_list_cmp(v, a, b);
        return c ? c < 0 : a < b;
    }
};

/* the output order of the groups' heads: their (distinct) lists alone */
struct UniqListLess {
    UniqLists v;
    __host__ __device__ bool operator()(uint32_t a, uint32_t b) const
    {
        if (a >= v.n || b >= v.n)
            return a < b;
        const int c = uniq_list_cmp(v, a, b);
        return c ? c < 0 : a < b;
    }
};

/* One wave per position of the sorted order: flag[p] = the sequence's list
 * differs from its predecessor's (position 0: set).  Sizes first, then 64
 * keys per step, one per lane, and a ballot. */
__global__ __launch_bounds__(256) void uniq_heads_kernel(UniqLists v, const uint32_t *__restrict__ order,
                                                         uint32_t *__restrict__ flag)
{
    const uint64_t p = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (p >= v.n)
        return;
    bool differ = true;
    if (p > 0) {
        const uint32_t a = order[p - 1], b = order[p];
        const uint64_t oa = v.set_off[a], ob = v.set_off[b];
        const uint64_t la = v.set_off[a + 1] - oa, lb = v.set_off[b + 1] - ob;
        differ = la != lb;
        if (!differ) {
            for (uint64_t base = 0; base < la; base += kUniqWaveStep) {
                const uint64_t k = base + lane_id();
                const bool ne = k < la && v.keys[oa + k] != v.keys[ob + k];
                if (__ballot(ne)) {
                    differ = true;
                    break;
                }
            }
        }
    }
    if (lane_id() == 0)
        flag[p] = differ;
}

/* per group g of the sorted order (head_pos: its first position): its head
 * sequence, its size, its own number */
__global__ __launch_bounds__(256) void uniq_group_heads_kernel(const uint32_t *__restrict__ order,
                                                               const uint32_t *__restrict__ head_pos, uint32_t n_groups,
                                                               uint32_t n, uint32_t *__restrict__ head_seq,
                                                               uint32_t *__restrict__ gsize, uint32_t *__restrict__ gid)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups)
        return;
    const uint32_t p = head_pos[g];
    head_seq[g] = order[p];
    gsize[g] = (g + 1 < n_groups ? head_pos[g + 1] : n) - p;
    gid[g] = (uint32_t)g;
}

/* per rank r of the output order (gid[r]: the group there, head_seq[r]: its
 * head): the group's rank, and the sizes the two CSRs are scanned from
 * (n_groups + 1 entries, the last 0) */
__global__ __launch_bounds__(256) void uniq_ranks_kernel(UniqLists v, const uint32_t *__restrict__ head_seq,
                                                         const uint32_t *__restrict__ gid,
                                                         const uint32_t *__restrict__ gsize, uint32_t n_groups,
                                                         uint32_t *__restrict__ rank_of, uint64_t *__restrict__ rsize,
                                                         uint64_t *__restrict__ rlen)
{
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > n_groups)
        return;
    if (r == n_groups) {
        rsize[r] = 0;
        rlen[r] = 0;
        return;
    }
    const uint32_t g = gid[r], s = head_seq[r];
    rank_of[g] = (uint32_t)r;
    rsize[r] = gsize[g];
    rlen[r] = v.set_off[s + 1] - v.set_off[s];
}

/* per position p of the sorted order (incl[p] - 1: its group there): the
 * sequence into its group's row -- positions within a group ascend by index --
 * and the group's rank into group_of */
__global__ __launch_bounds__(256) void uniq_members_kernel(const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ incl,
                                                           const uint32_t *__restrict__ head_pos,
                                                           const uint32_t *__restrict__ rank_of,
                                                           const uint64_t *__restrict__ goff, uint32_t n,
                                                           uint32_t *__restrict__ members, uint32_t *__restrict__ group_of)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n)
        return;
    const uint32_t g = incl[p] - 1u, r = rank_of[g], s = order[p];
    members[goff[r] + (p - head_pos[g])] = s;
    group_of[s] = r;
}

/* one wave per group of the output order: its head's list to the groups' keys */
__global__ __launch_bounds__(256) void uniq_gather_sets_kernel(UniqLists v, const uint32_t *__restrict__ head_seq,
                                                               const uint64_t *__restrict__ soff, uint32_t n_groups,
                                                               uint64_t *__restrict__ out)
{
    const uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (r >= n_groups)
        return;
    const uint32_t s = head_seq[r];
    const uint64_t a = v.set_off[s], len = v.set_off[s + 1] - a, to = soff[r];
    for (uint64_t k = lane_id(); k < len; k += kUniqWaveStep)
        out[to + k] = v.keys[a + k];
}

}  // namespace kgx

using namespace kgx;

struct kgx_uniq {
    kgx_uniq_stats stats{};
    std::vector<uint64_t> group_off{0}, set_off{0}, keys;
    std::vector<uint32_t> members, group_of;
};

namespace {

enum { kUp = 0, kPass, kSets, kGroup, kDown };

struct UniqEvents {
    hipEvent_t e[4] = {};
    ~UniqEvents()
    {
        for (hipEvent_t x : e)
            if (x)
                (void)hipEventDestroy(x);
    }
    int create()
    {
        for (hipEvent_t &x : e)
            HIP_TRY(hipEventCreate(&x));
        return KGX_OK;
    }
    /* the time between marks a and b (both reached) goes to stage s */
    int add(int a, int b, int s, float *ms)
    {
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, e[a], e[b]));
        ms[s] += t;
        return KGX_OK;
    }
};

dim3 uniq_grid(uint64_t threads) { return dim3((uint32_t)std::max<uint64_t>((threads + 255) / 256, 1)); }

int uniq_nomem(const char *what, uint64_t bytes)
{
    (void)hipGetLastError();
    return fail(KGX_ENOMEM, std::string("unique: the corpus' key lists do not fit the device: ") + what + " asked for " +
                                std::to_string(bytes) + " bytes");
}

#define UNIQ_ALLOC(buf, bytes)                                  \
    do {                                                        \
        const uint64_t b_ = (bytes);                            \
        if ((buf).reserve(b_) != hipSuccess)                    \
            return uniq_nomem(#buf, b_);                        \
    } while (0)

/* a hipCUB call, f(temporary storage, its size): asked for its size, then run */
template <class F> int uniq_cub(DevBuf &tmp, F f)
{
    size_t bytes = 0;
    HIP_TRY(f(nullptr, bytes));
    UNIQ_ALLOC(tmp, std::max<size_t>(bytes, 256)); /* never null: that asks for the size */
    HIP_TRY(f(tmp.p, bytes));
    return KGX_OK;
}

/* buf holds `used` bytes that stay; room for `need` */
int uniq_grow(DevBuf &buf, uint64_t used, uint64_t need, hipStream_t s)
{
    if (need <= buf.cap)
        return KGX_OK;
    DevBuf nb;
    if (nb.reserve(std::max<uint64_t>(need, 2 * (uint64_t)buf.cap)) != hipSuccess) {
        (void)hipGetLastError();
        if (nb.reserve(need) != hipSuccess)
            return uniq_nomem("keys", need);
    }
    if (used)
        HIP_TRY(hipMemcpyAsync(nb.p, buf.p, used, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); /* the old buffer goes with the swap */
    buf = std::move(nb);
    return KGX_OK;
}

struct UniqDev {
    DevBuf set_off, keys, counts, base, pairs, sorted, uq, n_sel, tmp;
    DevBuf digest, order, walks, flag, incl, head_pos, head_seq, gsize, gid, rank_of, rsize, rlen, goff, soff, members,
        group_of, gkeys;
};

/* one piece's hits (the context's current plan, m sequences from s0) into its
 * sequences' key lists, appended at *n_keys */
int uniq_piece_sets(kgx_ctx *c, UniqDev &D, uint32_t s0, uint32_t m, uint64_t *n_keys, uint64_t *n_hits)
{
    hipStream_t s = c->stream;
    const Tiled t = tiled_of(c);
    const uint64_t nt = c->max_tiles;
    uint64_t *set_off = D.set_off.as<uint64_t>() + s0;
    uint32_t total = 0;
    if (nt + 1 > 0x7FFFFFFFull)
        return fail(KGX_ERANGE, "unique: a piece of " + std::to_string(nt) + " tiles");
    UNIQ_ALLOC(D.counts, (nt + 1) * 4);
    UNIQ_ALLOC(D.base, (nt + 1) * 4);
    hipLaunchKernelGGL(uniq_tile_counts_kernel, uniq_grid(nt + 1), dim3(256), 0, s, t, nt, D.counts.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    int rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceScan::ExclusiveSum(p, b, D.counts.as<uint32_t>(), D.base.as<uint32_t>(), (int)(nt + 1), s);
    });
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(&total, D.base.as<uint32_t>() + nt, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (total > 0x7FFFFFFFu)
        return fail(KGX_ERANGE, "unique: a piece of " + std::to_string(total) + " hits");
    uint64_t n_u = 0;
    if (total) {
        UNIQ_ALLOC(D.pairs, (uint64_t)total * 8);
        UNIQ_ALLOC(D.sorted, (uint64_t)total * 8);
        UNIQ_ALLOC(D.uq, (uint64_t)total * 8);
        UNIQ_ALLOC(D.n_sel, 8);
        hipLaunchKernelGGL(uniq_pairs_kernel, uniq_grid(nt * t.T), dim3(256), 0, s, t, nt, D.base.as<uint32_t>(),
                           D.pairs.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        /* the bits in use: the key's 35 and what m - 1 needs */
        int seq_bits = 0;
        while (seq_bits < 29 && (1u << seq_bits) < m)
            seq_bits++;
        rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
            return hipcub::DeviceRadixSort::SortKeys(p, b, D.pairs.as<uint64_t>(), D.sorted.as<uint64_t>(), (int)total, 0,
                                                     (int)kUniqKeyBits + seq_bits, s);
        });
        if (rc)
            return rc;
        rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
            return hipcub::DeviceSelect::Unique(p, b, D.sorted.as<uint64_t>(), D.uq.as<uint64_t>(),
                                                D.n_sel.as<unsigned long long>(), (int)total, s);
        });
        if (rc)
            return rc;
        unsigned long long h_n = 0;
        HIP_TRY(hipMemcpyAsync(&h_n, D.n_sel.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_n == 0 || h_n > total)
            return fail(KGX_EDEVICE, "unique: bad list sizes");
        n_u = h_n;
        if ((rc = uniq_grow(D.keys, *n_keys * 8, (*n_keys + n_u) * 8, s)))
            return rc;
        hipLaunchKernelGGL(uniq_strip_kernel, uniq_grid(n_u), dim3(256), 0, s, D.uq.as<uint64_t>(), n_u,
                           D.keys.as<uint64_t>() + *n_keys);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(uniq_set_off_kernel, uniq_grid((uint64_t)m + 1), dim3(256), 0, s, D.uq.as<uint64_t>(), n_u, m,
                       *n_keys, set_off);
    HIP_TRY(hipGetLastError());
    *n_keys += n_u;
    *n_hits += total;
    return KGX_OK;
}

/* the corpus' lists (D.set_off, D.keys) into groups, and those to the host */
int uniq_group(kgx_ctx *c, UniqDev &D, uint32_t n, uint64_t n_keys, uint32_t digest_bits, UniqEvents &ev, kgx_uniq *U)
{
    hipStream_t s = c->stream;
    kgx_uniq_stats &st = U->stats;
    int rc;
    HIP_TRY(hipEventRecord(ev.e[0], s));
    UNIQ_ALLOC(D.keys, std::max<uint64_t>(n_keys, 1) * 8);
    UNIQ_ALLOC(D.digest, (uint64_t)n * 8);
    UNIQ_ALLOC(D.order, (uint64_t)n * 4);
    UNIQ_ALLOC(D.walks, 16);
    UNIQ_ALLOC(D.flag, (uint64_t)n * 4);
    UNIQ_ALLOC(D.incl, (uint64_t)n * 4);
    UNIQ_ALLOC(D.head_pos, (uint64_t)n * 4);
    UNIQ_ALLOC(D.n_sel, 8);
    HIP_TRY(hipMemsetAsync(D.walks.p, 0, 16, s));
    const uint64_t mask = digest_bits >= 64 ? ~0ull : ((1ull << digest_bits) - 1);
    hipLaunchKernelGGL(uniq_digest_thread_kernel, uniq_grid(n), dim3(256), 0, s, D.set_off.as<uint64_t>(),
                       D.keys.as<uint64_t>(), n, mask, D.digest.as<uint64_t>());
    hipLaunchKernelGGL(uniq_digest_wave_kernel, uniq_grid((uint64_t)n * 64), dim3(256), 0, s, D.set_off.as<uint64_t>(),
                       D.keys.as<uint64_t>(), n, mask, D.digest.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    const UniqLists v{D.set_off.as<uint64_t>(), D.keys.as<uint64_t>(), D.digest.as<uint64_t>(), n};
    /* the grouping order */
    hipcub::CountingInputIterator<uint32_t> ids(0);
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceMergeSort::SortKeysCopy(p, b, ids, D.order.as<uint32_t>(), (int)n,
                                                     UniqGroupLess{v, D.walks.as<unsigned long long>()}, s);
    });
    if (rc)
        return rc;
    /* heads, group ids, head positions */
    hipLaunchKernelGGL(uniq_heads_kernel, uniq_grid((uint64_t)n * 64), dim3(256), 0, s, v, D.order.as<uint32_t>(),
                       D.flag.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceScan::InclusiveSum(p, b, D.flag.as<uint32_t>(), D.incl.as<uint32_t>(), (int)n, s);
    });
    if (rc)
        return rc;
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceSelect::Flagged(p, b, ids, D.flag.as<uint32_t>(), D.head_pos.as<uint32_t>(),
                                             D.n_sel.as<unsigned long long>(), (int)n, s);
    });
    if (rc)
        return rc;
    unsigned long long h_g = 0;
    HIP_TRY(hipMemcpyAsync(&h_g, D.n_sel.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_g == 0 || h_g > n)
        return fail(KGX_EDEVICE, "unique: bad group count");
    const uint32_t G = (uint32_t)h_g;
    /* the output order of the groups, and the two CSRs' offsets */
    UNIQ_ALLOC(D.head_seq, (uint64_t)G * 4);
    UNIQ_ALLOC(D.gsize, (uint64_t)G * 4);
    UNIQ_ALLOC(D.gid, (uint64_t)G * 4);
    UNIQ_ALLOC(D.rank_of, (uint64_t)G * 4);
    UNIQ_ALLOC(D.rsize, ((uint64_t)G + 1) * 8);
    UNIQ_ALLOC(D.rlen, ((uint64_t)G + 1) * 8);
    UNIQ_ALLOC(D.goff, ((uint64_t)G + 1) * 8);
    UNIQ_ALLOC(D.soff, ((uint64_t)G + 1) * 8);
    UNIQ_ALLOC(D.members, (uint64_t)n * 4);
    UNIQ_ALLOC(D.group_of, (uint64_t)n * 4);
    hipLaunchKernelGGL(uniq_group_heads_kernel, uniq_grid(G), dim3(256), 0, s, D.order.as<uint32_t>(),
                       D.head_pos.as<uint32_t>(), G, n, D.head_seq.as<uint32_t>(), D.gsize.as<uint32_t>(),
                       D.gid.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceMergeSort::SortPairs(p, b, D.head_seq.as<uint32_t>(), D.gid.as<uint32_t>(), (int)G,
                                                  UniqListLess{v}, s);
    });
    if (rc)
        return rc;
    hipLaunchKernelGGL(uniq_ranks_kernel, uniq_grid((uint64_t)G + 1), dim3(256), 0, s, v, D.head_seq.as<uint32_t>(),
                       D.gid.as<uint32_t>(), D.gsize.as<uint32_t>(), G, D.rank_of.as<uint32_t>(), D.rsize.as<uint64_t>(),
                       D.rlen.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceScan::ExclusiveSum(p, b, D.rsize.as<uint64_t>(), D.goff.as<uint64_t>(), (int)(G + 1u), s);
    });
    if (rc)
        return rc;
    rc = uniq_cub(D.tmp, [&](void *p, size_t &b) {
        return hipcub::DeviceScan::ExclusiveSum(p, b, D.rlen.as<uint64_t>(), D.soff.as<uint64_t>(), (int)(G + 1u), s);
    });
    if (rc)
        return rc;
    hipLaunchKernelGGL(uniq_members_kernel, uniq_grid(n), dim3(256), 0, s, D.order.as<uint32_t>(), D.incl.as<uint32_t>(),
                       D.head_pos.as<uint32_t>(), D.rank_of.as<uint32_t>(), D.goff.as<uint64_t>(), n,
                       D.members.as<uint32_t>(), D.group_of.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    uint64_t n_gkeys = 0;
    HIP_TRY(hipMemcpyAsync(&n_gkeys, D.soff.as<uint64_t>() + G, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (n_gkeys > n_keys)
        return fail(KGX_EDEVICE, "unique: bad key count");
    UNIQ_ALLOC(D.gkeys, std::max<uint64_t>(n_gkeys, 1) * 8);
    hipLaunchKernelGGL(uniq_gather_sets_kernel, uniq_grid((uint64_t)G * 64), dim3(256), 0, s, v, D.head_seq.as<uint32_t>(),
                       D.soff.as<uint64_t>(), G, D.gkeys.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev.e[1], s));

    /* download */
    U->group_off.resize((size_t)G + 1);
    U->set_off.resize((size_t)G + 1);
    U->members.resize(n);
    U->group_of.resize(n);
    U->keys.resize(n_gkeys);
    unsigned long long walks = 0;
    HIP_TRY(hipMemcpyAsync(U->group_off.data(), D.goff.p, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(U->set_off.data(), D.soff.p, ((size_t)G + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(U->members.data(), D.members.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(U->group_of.data(), D.group_of.p, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (n_gkeys)
        HIP_TRY(hipMemcpyAsync(U->keys.data(), D.gkeys.p, n_gkeys * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&walks, D.walks.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(ev.e[2], s));
    HIP_TRY(hipStreamSynchronize(s));
    if ((rc = ev.add(0, 1, kGroup, st.stage_ms)) || (rc = ev.add(1, 2, kDown, st.stage_ms)))
        return rc;
    if (U->group_off[G] != n)
        return fail(KGX_EDEVICE, "unique: the groups do not hold every sequence");
    st.n_groups = G;
    st.list_compares = walks;
    for (uint32_t r = 0; r < G; r++)
        st.largest_group = std::max<uint64_t>(st.largest_group, U->group_off[r + 1] - U->group_off[r]);
    st.n_empty = U->set_off[1] == 0 ? U->group_off[1] : 0;
    return KGX_OK;
}

int uniq_run(kgx_ctx *c, const char *residues, const uint64_t *off, uint32_t n_seq, uint64_t piece_residues,
             uint32_t digest_bits, kgx_uniq *U)
{
    kgx_uniq_stats &st = U->stats;
    st.n_seq = n_seq;
    st.digest_bits = digest_bits;
    if (n_seq == 0)
        return KGX_OK;
    hipStream_t s = c->stream;
    UniqEvents ev;
    int rc = ev.create();
    if (rc)
        return rc;
    UniqDev D;
    UNIQ_ALLOC(D.set_off, ((uint64_t)n_seq + 1) * 8);
    UNIQ_ALLOC(D.uq, 256); /* a piece without hits still hands the pointer on */
    uint64_t n_keys = 0, n_hits = 0;

    /* the pieces, one after the other: stage, upload, plan and probe, sets */
    for (uint32_t s0 = 0; s0 < n_seq;) {
        uint32_t s1 = s0 + 1;
        while (s1 < n_seq && s1 - s0 < kUniqPieceSeqs && off[s1 + 1] - off[s0] <= piece_residues)
            s1++;
        const uint32_t m = s1 - s0;
        const uint64_t r0 = off[s0], n_res = off[s1] - r0;
        /* hits <= windows < residues: what one hipCUB call counts */
        if (n_res > 0x7FFFFFFFull)
            return fail(KGX_ERANGE, "unique: a piece of " + std::to_string(n_res) + " residues");
        HIP_TRY(hipEventRecord(ev.e[0], s));
        HIP_TRY(c->h_res.resize(n_res));
        HIP_TRY(c->h_off_stage.resize(m + 1));
        for (uint32_t i = 0; i <= m; i++)
            c->h_off_stage[i] = off[s0 + i] - r0;
        HIP_TRY(c->residues.reserve(n_res + 16));
        HIP_TRY(c->offsets.reserve((m + 1ull) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(c->offsets.p, c->h_off_stage.data(), (m + 1ull) * sizeof(uint64_t), hipMemcpyHostToDevice,
                               s));
        if ((rc = recall_stage_upload(c, residues + r0, n_res, off + s0, m)))
            return rc;
        HIP_TRY(hipEventRecord(ev.e[1], s));
        /* hits only: no scorer runs */
        if ((rc = kgx_stage_plan(c, c->offsets.as<uint64_t>(), m, n_res)) ||
            (rc = kgx_stage_probe(c, c->residues.as<uint8_t>(), c->offsets.as<uint64_t>())))
            return rc;
        if (!c->have_hits)
            return fail(KGX_EDEVICE, "unique: the probe left no hits");
        HIP_TRY(hipEventRecord(ev.e[2], s));
        if ((rc = uniq_piece_sets(c, D, s0, m, &n_keys, &n_hits)))
            return rc;
        HIP_TRY(hipEventRecord(ev.e[3], s));
        /* the staging buffers and the context's arrays are the next piece's too */
        HIP_TRY(hipStreamSynchronize(s));
        if ((rc = ev.add(0, 1, kUp, st.stage_ms)) || (rc = ev.add(1, 2, kPass, st.stage_ms)) ||
            (rc = ev.add(2, 3, kSets, st.stage_ms)))
            return rc;
        st.n_pieces++;
        s0 = s1;
    }
    st.n_hits = n_hits;
    st.n_set_keys = n_keys;
    return uniq_group(c, D, n_seq, n_keys, digest_bits, ev, U);
}

}  // namespace

extern "C" {

int kgx_uniq_run(kgx_ctx *c, const char *residues, const uint64_t *seq_offsets, uint32_t n_seq,
                 uint64_t piece_residues, uint32_t digest_bits, kgx_uniq **out)
{
    if (!out)
        return fail(KGX_EINVAL, "null argument");
    *out = nullptr;
    if (digest_bits > 64)
        return fail(KGX_EINVAL, "unique: digest_bits = " + std::to_string(digest_bits) + " is above 64");
    if (!c || !c->img || !seq_offsets)
        return fail(KGX_EINVAL, "null argument");
    if (n_seq > 0x7FFFFFFFu) /* hipCUB counts items in an int */
        return fail(KGX_ERANGE, "unique: more than 2^31-1 sequences");
    for (uint32_t i = 0; i < n_seq; i++)
        if (seq_offsets[i + 1] < seq_offsets[i])
            return fail(KGX_EINVAL, "seq_offsets not monotone");
    if (n_seq && seq_offsets[n_seq] > seq_offsets[0] && !residues)
        return fail(KGX_EINVAL, "null residues");
    if (!is_gfx950(c->img->device))
        return fail(KGX_EDEVICE, "device " + std::to_string(c->img->device) + " is not gfx950");
    HIP_TRY(hipSetDevice(c->img->device));
    kgx_uniq *U = new kgx_uniq;
    const int rc = uniq_run(c, residues, seq_offsets, n_seq, piece_residues ? piece_residues : kUniqPiece, digest_bits, U);
    if (rc) {
        (void)hipStreamSynchronize(c->stream); /* nothing of this call is in flight when its arrays go */
        delete U;
        return rc;
    }
    *out = U;
    return KGX_OK;
}

int kgx_uniq_stats_get(const kgx_uniq *u, kgx_uniq_stats *out)
{
    if (!u || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = u->stats;
    return KGX_OK;
}

int kgx_uniq_groups(const kgx_uniq *u, const uint64_t **group_offsets, const uint32_t **members, uint64_t *n_groups)
{
    if (!u || !group_offsets || !members || !n_groups)
        return fail(KGX_EINVAL, "null argument");
    *group_offsets = u->group_off.data();
    *members = u->members.data();
    *n_groups = u->group_off.size() - 1;
    return KGX_OK;
}

int kgx_uniq_group_of(const kgx_uniq *u, const uint32_t **group, uint64_t *n_seq)
{
    if (!u || !group || !n_seq)
        return fail(KGX_EINVAL, "null argument");
    *group = u->group_of.data();
    *n_seq = u->group_of.size();
    return KGX_OK;
}

int kgx_uniq_sets(const kgx_uniq *u, const uint64_t **set_offsets, const uint64_t **keys, uint64_t *n_groups)
{
    if (!u || !set_offsets || !keys || !n_groups)
        return fail(KGX_EINVAL, "null argument");
    *set_offsets = u->set_off.data();
    *keys = u->keys.data();
    *n_groups = u->set_off.size() - 1;
    return KGX_OK;
}

int kgx_uniq_destroy(kgx_uniq *u)
{
    delete u;
    return KGX_OK;
}

} /* extern "C" */
