/*
 * kgx_fq_ids.hip -- the ids of chosen reads of a device parse (include/kgx.h
 * kgx_fq_read_ids).  kgx_fq_parse leaves every read's id in
 * HBM; the fq handler prints the ids of the reads that score, a sparse subset,
 * so only those come down:
 *
 *   len    per chosen read its id's length; a workgroup's 256 lengths scanned
 *          (wave_scan_add, then the four waves through LDS): each read's offset
 *          within its tile, and the tile's sum
 *   sums   one workgroup: the exclusive sums of the tiles' sums and the total
 *          (sums_body, the parser's own, over x alone)
 *   copy   16 lanes move one id byte by byte to its place, a longer id in
 *          rounds of 16; lane 0 of the group writes the id's offset
 *
 * and the offsets and bytes are downloaded into pinned memory.  Separate
 * launches: no kernel waits on another workgroup.
 */
#include "kgx_device.h"
#include "kgx_rt.h"
#include "kgx_text_scan.h"

using namespace kgx;
using namespace kgx::text_scan;

namespace {

constexpr uint32_t IDS_TILE = WG;  /* chosen reads per workgroup of the length pass */
constexpr uint32_t IDS_GROUP = 16; /* lanes that move one id */

/* 1. lengths, their exclusive sums within the tile, the tile's sum */
__global__ __launch_bounds__(256) void fq_ids_len_kernel(const uint64_t *__restrict__ id_offsets,
                                                         const uint32_t *__restrict__ read_index, uint32_t n,
                                                         uint32_t *__restrict__ local_off, uint4 *__restrict__ tile_cnt)
{
    __shared__ uint32_t wave_sum[WAVES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint64_t i = (uint64_t)blockIdx.x * IDS_TILE + tid;
    uint32_t len = 0;
    if (i < n) {
        const uint32_t r = read_index[i];
        len = (uint32_t)(id_offsets[(uint64_t)r + 1] - id_offsets[r]);
    }
    const uint32_t inc = wave_scan_add(len, lane);
    if (lane == 63)
        wave_sum[wv] = inc;
    __syncthreads();
    uint32_t before = inc - len, total = 0;
    for (uint32_t k = 0; k < WAVES; k++) {
        if (k < wv)
            before += wave_sum[k];
        total += wave_sum[k];
    }
    if (i < n)
        local_off[i] = before;
    if (tid == 0)
        tile_cnt[blockIdx.x] = make_uint4(total, 0, 0, 0);
}

/* 2. one workgroup: the tiles' exclusive sums (x) and the total in sums[SUM_IDS] */
__global__ __launch_bounds__(256) void fq_ids_sums_kernel(const uint4 *__restrict__ tile_cnt, uint32_t n_tiles,
                                                          uint4 *__restrict__ tile_pre, uint64_t *sums)
{
    sums_body(tile_cnt, n_tiles, tile_pre, sums);
}

/* 3. the ids to their places.  Loads stay inside ids[0, n_id_bytes) and
 * stores inside out[0, n_id_bytes): an id that would not (offsets that are
 * not the parse's) is not moved */
__global__ __launch_bounds__(256) void fq_ids_copy_kernel(const uint8_t *__restrict__ ids,
                                                          const uint64_t *__restrict__ id_offsets,
                                                          const uint32_t *__restrict__ read_index, uint32_t n,
                                                          const uint32_t *__restrict__ local_off,
                                                          const uint4 *__restrict__ tile_pre, uint64_t n_id_bytes,
                                                          uint8_t *__restrict__ out, uint64_t *__restrict__ out_off)
{
    const uint64_t i = (uint64_t)blockIdx.x * (WG / IDS_GROUP) + threadIdx.x / IDS_GROUP;
    const uint32_t g = threadIdx.x % IDS_GROUP;
    if (i >= n)
        return;
    const uint32_t r = read_index[i];
    const uint64_t a = id_offsets[r], b = id_offsets[(uint64_t)r + 1];
    const uint64_t at = (uint64_t)tile_pre[i / IDS_TILE].x + local_off[i];
    const uint64_t len = b >= a ? b - a : 0;
    if (g == 0) {
        out_off[i] = at;
        if (i + 1 == n)
            out_off[n] = at + len;
    }
    if (b > n_id_bytes || at + len > n_id_bytes)
        return;
    for (uint64_t j = g; j < len; j += IDS_GROUP)
        out[at + j] = ids[a + j];
}

/* reads is what this context's last kgx_fq_parse[_device] returned: the check
 * kgx_fq_proteins_device makes, and the counts of that call */
bool last_parse(const kgx_ctx *c, const kgx_fq_reads *r)
{
    const kgx_fq_reads &l = c->fp_last;
    if (r->n_reads != l.n_reads || r->n_bases != l.n_bases || r->n_id_bytes != l.n_id_bytes ||
        r->consumed != l.consumed || r->bases != l.bases || r->read_offsets != l.read_offsets || r->ids != l.ids ||
        r->id_offsets != l.id_offsets)
        return false;
    if (!r->n_reads)
        return true;
    return r->bases == c->fq_bases.p && r->read_offsets == c->fq_roff.p && r->ids == c->ft_ids.p &&
           r->id_offsets == c->ft_idoff.p && r->n_id_bytes + 16 <= c->ft_ids.cap &&
           ((uint64_t)r->n_reads + 1) * 8 <= c->ft_idoff.cap;
}

}  // namespace

extern "C" {

int kgx_fq_read_ids(kgx_ctx *c, const kgx_fq_reads *reads, const uint32_t *read_index, uint32_t n, kgx_fq_ids *out)
{
    static const uint64_t zero = 0;
    if (!c || !reads || !out || (n && !read_index))
        return fail(KGX_EINVAL, "null argument");
    *out = kgx_fq_ids{0, 0, "", &zero};
    if (!last_parse(c, reads))
        return fail(KGX_EINVAL, "kgx_fq_read_ids: not the reads of this context's last kgx_fq_parse call");
    for (uint32_t i = 0; i < n; i++) {
        if (read_index[i] >= reads->n_reads)
            return fail(KGX_EINVAL, "kgx_fq_read_ids: read index " + std::to_string(read_index[i]) + " of " +
                                        std::to_string(reads->n_reads) + " reads");
        if (i && read_index[i] <= read_index[i - 1])
            return fail(KGX_EINVAL, "kgx_fq_read_ids: read_index is not strictly ascending");
    }
    if (!n)
        return KGX_OK;
    HIP_TRY(hipSetDevice(c->img->device));
    hipStream_t st = c->stream;
    const uint32_t n_tiles = (uint32_t)(((uint64_t)n + IDS_TILE - 1) / IDS_TILE);
    HIP_TRY(c->fi_index.reserve((uint64_t)n * 4));
    HIP_TRY(c->fi_local.reserve((uint64_t)n * 4));
    HIP_TRY(c->fi_cnt.reserve((uint64_t)n_tiles * 16));
    HIP_TRY(c->fi_pre.reserve((uint64_t)n_tiles * 16));
    HIP_TRY(c->fi_sum.reserve(SUM_WORDS * 8));
    HIP_TRY(c->fi_off.reserve(((uint64_t)n + 1) * 8));
    HIP_TRY(c->fi_ids.reserve(reads->n_id_bytes + 16)); /* distinct reads: no more than every id byte */
    HIP_TRY(c->h_fi_index.resize(n));
    HIP_TRY(c->h_fi_off.resize((uint64_t)n + 1));
    std::memcpy(c->h_fi_index.data(), read_index, (size_t)n * 4);
    HIP_TRY(hipMemcpyAsync(c->fi_index.p, c->h_fi_index.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(fq_ids_len_kernel, dim3(n_tiles), dim3(WG), 0, st, reads->id_offsets, c->fi_index.as<uint32_t>(),
                       n, c->fi_local.as<uint32_t>(), c->fi_cnt.as<uint4>());
    hipLaunchKernelGGL(fq_ids_sums_kernel, dim3(1), dim3(WG), 0, st, c->fi_cnt.as<uint4>(), n_tiles,
                       c->fi_pre.as<uint4>(), c->fi_sum.as<uint64_t>());
    hipLaunchKernelGGL(fq_ids_copy_kernel, dim3((uint32_t)(((uint64_t)n + WG / IDS_GROUP - 1) / (WG / IDS_GROUP))),
                       dim3(WG), 0, st, reads->ids, reads->id_offsets, c->fi_index.as<uint32_t>(), n,
                       c->fi_local.as<uint32_t>(), c->fi_pre.as<uint4>(), reads->n_id_bytes, c->fi_ids.as<uint8_t>(),
                       c->fi_off.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_fi_off.data(), c->fi_off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(host_wait(st));
    const uint64_t total = c->h_fi_off[n];
    if (total > reads->n_id_bytes)
        return fail(KGX_EDEVICE, "kgx_fq_read_ids: more id bytes than the parse left");
    HIP_TRY(c->h_fi_ids.resize(total + 1));
    if (total) {
        HIP_TRY(hipMemcpyAsync(c->h_fi_ids.data(), c->fi_ids.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(host_wait(st));
    }
    c->fq_ids_fetched += n;
    out->n = n;
    out->n_bytes = total;
    out->ids = c->h_fi_ids.data();
    out->id_offsets = c->h_fi_off.data();
    return KGX_OK;
}

}  // extern "C"
