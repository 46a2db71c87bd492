/*
 * kgx_fa_parse.hip -- the FASTA parser on the device (include/kgx.h
 * kgx_fa_parse*): text in device memory -> residues,
 * seq_offsets, ids, id_offsets in buffers of the context's own, the first two
 * as kgx_run_device takes them.
 *
 * The parser is FastaParser::parse_char (fasta_parser.h:38-144): five states
 * (start, id, defline, data, id-or-data) over seven byte classes ('\n', '\r',
 * '>', blank, '*', ASCII letter, other).  '\r' is transparent: its map is the
 * identity and it has no event in any state.  A record ends at the '>' that
 * opens the next one, so that byte is not consumed with the record it ends.
 * The scan is kgx_text_scan.h's, the one the FASTQ parser uses
 * (kgx_fq_parse.hip), with this file's machine: map, state, count, sums,
 * write, no_id as separate launches over 4096-byte tiles, and the scratch
 * buffers (fp_*) and the text staging are that parser's too.
 *
 * Strict mode is the lenient machine cut at the first offending byte e: the
 * host reads e with the totals and, when there is one, runs count and sums
 * again over [0, e).  The tiles' entry states do not depend on what follows
 * them.
 */
#include "kgx_device.h"
#include "kgx_rt.h"
#include "kgx_text_scan.h"

using namespace kgx;
using namespace kgx::text_scan;

namespace {

struct FaMachine {
    enum : uint32_t { S_START, S_ID, S_DEF, S_DATA, S_ID_OR_DATA, N_STATES };
    enum : uint32_t { C_NL, C_CR, C_GT, C_BLANK, C_STAR, C_LETTER, C_OTHER, N_CLASSES };
    static constexpr uint32_t END_TAKES_BYTE = 0; /* the '>' that ends a record opens the next */

    static constexpr uint32_t next_state(uint32_t s, uint32_t c)
    {
        if (c == C_CR)
            return s;
        switch (s) {
        case S_START: return c == C_GT ? S_ID : S_START;
        case S_ID: return c == C_BLANK ? S_DEF : c == C_NL ? S_DATA : S_ID;
        case S_DEF: return c == C_NL ? S_DATA : S_DEF;
        case S_DATA: return c == C_NL ? S_ID_OR_DATA : S_DATA;
        default: return c == C_GT ? S_ID : c == C_LETTER ? S_DATA : S_ID_OR_DATA;
        }
    }

    static constexpr uint32_t event_of(uint32_t s, uint32_t c)
    {
        if (c == C_CR)
            return 0;
        switch (s) {
        case S_START: return c == C_GT ? 0 : EV_BAD;
        case S_ID: return (c == C_NL || c == C_BLANK) ? 0 : EV_ID;
        case S_DEF: return 0;
        case S_DATA: return c == C_NL ? 0 : (c == C_LETTER || c == C_STAR) ? EV_DATA : EV_BAD;
        default: return c == C_GT ? EV_END : c == C_NL ? 0 : c == C_LETTER ? EV_DATA : EV_BAD;
        }
    }

    /* isblank and isalpha in the C locale; bytes >= 0x80 are "other" */
    static __device__ __forceinline__ uint32_t class_of(uint32_t b)
    {
        const bool letter = ((b | 0x20u) - 'a') < 26u;
        return b == '\n' ? C_NL
               : b == '\r' ? C_CR
               : b == '>' ? C_GT
               : (b == ' ' || b == '\t') ? C_BLANK
               : b == '*' ? C_STAR
               : letter ? C_LETTER
                        : C_OTHER;
    }

    /* kgx_fa_seqs.error */
    static __device__ __forceinline__ uint32_t error_code(uint32_t s, uint32_t)
    {
        return s == S_START ? 1u : s == S_DATA ? 2u : 3u;
    }
};

/* 1. a tile's map */
__global__ __launch_bounds__(256) void fa_parse_map_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                           uint32_t *__restrict__ tile_map)
{
    map_body<FaMachine>(text, n, tile_map);
}

/* 2. one workgroup: every tile's entry state */
__global__ __launch_bounds__(256) void fa_parse_state_kernel(const uint32_t *__restrict__ tile_map, uint32_t n_tiles,
                                                             uint8_t *__restrict__ tile_state)
{
    state_body<FaMachine>(tile_map, n_tiles, tile_state);
}

/* 3. the lanes' entry states, the tile's counts, the first offending byte */
__global__ __launch_bounds__(256) void fa_parse_count_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                             const uint8_t *__restrict__ tile_state,
                                                             uint8_t *__restrict__ lane_state,
                                                             uint4 *__restrict__ tile_cnt, uint64_t *error_key)
{
    count_body<FaMachine>(text, n, tile_state, lane_state, tile_cnt, error_key);
}

/* 4. one workgroup: the exclusive sums of the tiles' counts, the call's sums */
__global__ __launch_bounds__(256) void fa_parse_sums_kernel(const uint4 *__restrict__ tile_cnt, uint32_t n_tiles,
                                                            uint4 *__restrict__ tile_pre, uint64_t *sums)
{
    sums_body(tile_cnt, n_tiles, tile_pre, sums);
}

/* 5. the outputs: seq_offsets and id_offsets hold n_records + 2 entries, the
 * record in progress at n closed by the totals */
__global__ __launch_bounds__(256) void fa_parse_write_kernel(
    const uint8_t *__restrict__ text, uint64_t n, const uint8_t *__restrict__ lane_state,
    const uint4 *__restrict__ tile_pre, uint32_t n_records, uint64_t n_ids, uint64_t n_residues, uint64_t error_pos,
    uint8_t *__restrict__ residues, uint64_t *__restrict__ seq_offsets, uint8_t *__restrict__ ids,
    uint64_t *__restrict__ id_offsets, uint64_t *sums)
{
    write_body<FaMachine>(text, n, lane_state, tile_pre, n_records, n_ids, n_residues, error_pos, residues, seq_offsets,
                          ids, id_offsets, sums);
}

/* 6. the records without an id */
__global__ __launch_bounds__(256) void fa_parse_no_id_kernel(const uint64_t *__restrict__ id_offsets, uint32_t n_records,
                                                             uint64_t *sums)
{
    no_id_body(id_offsets, n_records, sums);
}

/* count and sums over [0, n), and the sums read on the host */
int count_and_sum(kgx_ctx *c, const uint8_t *text, uint64_t n)
{
    hipStream_t st = c->stream;
    const uint32_t n_tiles = tiles_of(n);
    uint64_t *sums = c->fp_sum.as<uint64_t>();
    if (n_tiles)
        hipLaunchKernelGGL(fa_parse_count_kernel, dim3(n_tiles), dim3(WG), 0, st, text, n, c->fp_state.as<uint8_t>(),
                           c->fp_lane.as<uint8_t>(), c->fp_cnt.as<uint4>(), sums + SUM_ERROR_KEY);
    hipLaunchKernelGGL(fa_parse_sums_kernel, dim3(1), dim3(WG), 0, st, c->fp_cnt.as<uint4>(), n_tiles,
                       c->fp_pre.as<uint4>(), sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_fp_sum.data(), sums, (SUM_ERROR + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(host_wait(st));
    return KGX_OK;
}

/* kgx_fa_parse_device behind its argument checks (n > 0, or n = 0 under
 * KGX_FA_FINISHED: the one empty record); upload_ms is the caller's */
int fa_parse_device(kgx_ctx *c, const uint8_t *text, uint64_t n, uint32_t flags, kgx_fa_seqs *out)
{
    hipStream_t st = c->stream;
    const uint32_t n_tiles = tiles_of(n);
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
    if (n_tiles)
        hipLaunchKernelGGL(fa_parse_map_kernel, dim3(n_tiles), dim3(WG), 0, st, text, n, c->fp_map.as<uint32_t>());
    hipLaunchKernelGGL(fa_parse_state_kernel, dim3(1), dim3(WG), 0, st, c->fp_map.as<uint32_t>(), n_tiles,
                       c->fp_state.as<uint8_t>());
    HIP_TRY(hipGetLastError());
    if (int rc = count_and_sum(c, text, n))
        return rc;
    const uint64_t key = h[SUM_ERROR], all_newlines = h[SUM_NEWLINES];
    const bool offending = key != NO_ERROR;
    const uint64_t e = key >> 16;
    const bool cut = (flags & KGX_FA_STRICT) && offending;
    uint64_t n_eff = n;
    if (cut) { /* the machine over [0, e) */
        n_eff = e;
        if (int rc = count_and_sum(c, text, n_eff))
            return rc;
    }
    const uint64_t n_ids = h[SUM_IDS], n_res = h[SUM_DATA], n_rec = h[SUM_RECORDS], cut_newlines = h[SUM_NEWLINES];
    if (n_rec + 1 > UINT32_MAX || n_ids > n || n_res > n)
        return fail(KGX_EDEVICE, "kgx_fa_parse: sums beyond what the text allows");
    HIP_TRY(c->fa_res.reserve(n_res + 16));
    HIP_TRY(c->fa_soff.reserve((n_rec + 2) * 8));
    HIP_TRY(c->fa_ids.reserve(n_ids + 16));
    HIP_TRY(c->fa_idoff.reserve((n_rec + 2) * 8));
    hipLaunchKernelGGL(fa_parse_write_kernel, dim3(std::max<uint32_t>(1, tiles_of(n_eff))), dim3(WG), 0, st, text, n_eff,
                       c->fp_lane.as<uint8_t>(), c->fp_pre.as<uint4>(), (uint32_t)n_rec, n_ids, n_res,
                       (offending && !cut) ? e : NO_ERROR, c->fa_res.as<uint8_t>(), c->fa_soff.as<uint64_t>(),
                       c->fa_ids.as<uint8_t>(), c->fa_idoff.as<uint64_t>(), sums);
    if (n_rec)
        hipLaunchKernelGGL(fa_parse_no_id_kernel, dim3((uint32_t)((n_rec + WG - 1) / WG)), dim3(WG), 0, st,
                           c->fa_idoff.as<uint64_t>(), (uint32_t)n_rec, sums);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->fp_events[2], st));
    HIP_TRY(hipMemcpyAsync(h + SUM_CONSUMED, sums + SUM_CONSUMED, (SUM_NO_ID - SUM_CONSUMED + 1) * 8,
                           hipMemcpyDeviceToHost, st));
    HIP_TRY(host_wait(st));
    HIP_TRY(hipEventElapsedTime(&out->parse_ms, c->fp_events[1], c->fp_events[2]));

    /* the record in progress at the end of [0, n_eff): parse_complete hands it
     * over whatever it holds */
    const bool tail = cut || (flags & KGX_FA_FINISHED);
    const uint64_t tail_ids = n_ids - h[SUM_IDS_AT_END];
    out->n_seqs = (uint32_t)(n_rec + tail);
    out->n_seqs_no_id = (uint32_t)(h[SUM_NO_ID] + (tail && !tail_ids));
    out->n_residues = tail ? n_res : h[SUM_DATA_AT_END];
    out->n_id_bytes = tail ? n_ids : h[SUM_IDS_AT_END];
    out->residues = c->fa_res.as<uint8_t>();
    out->seq_offsets = c->fa_soff.as<uint64_t>();
    out->ids = c->fa_ids.as<uint8_t>();
    out->id_offsets = c->fa_idoff.as<uint64_t>();
    out->consumed = tail ? n : h[SUM_CONSUMED];
    out->newlines = tail ? all_newlines : h[SUM_CONSUMED_NL];
    if (offending && (cut || e < out->consumed)) {
        out->error = (uint32_t)(key >> 8 & 255u);
        out->error_byte = (uint32_t)(key & 255u);
        out->error_pos = e;
        out->error_newlines = cut ? cut_newlines + (out->error_byte == '\n') : h[SUM_ERROR_NL];
    }
    return KGX_OK;
}

int parse_checks(kgx_ctx *c, const void *text, uint64_t n, uint32_t flags, kgx_fa_seqs *out)
{
    if (!c || !out || (n && !text))
        return fail(KGX_EINVAL, "null argument");
    *out = kgx_fa_seqs{};
    if (flags & ~(KGX_FA_STRICT | KGX_FA_FINISHED))
        return fail(KGX_EINVAL, "kgx_fa_parse: flags are KGX_FA_STRICT and KGX_FA_FINISHED");
    if (n > KGX_FA_PARSE_MAX)
        return fail(KGX_ERANGE, "kgx_fa_parse: more than KGX_FA_PARSE_MAX bytes of text in one call");
    HIP_TRY(hipSetDevice(c->img->device));
    return ensure_events(c->fp_events, 3, hipEventDefault);
}

}  // namespace

extern "C" {

int kgx_fa_parse_device(kgx_ctx *c, const void *d_text, uint64_t n, uint32_t flags, kgx_fa_seqs *out)
{
    if (int rc = parse_checks(c, d_text, n, flags, out))
        return rc;
    if (!n && !(flags & KGX_FA_FINISHED))
        return KGX_OK;
    if (n && (reinterpret_cast<uintptr_t>(d_text) & 15u))
        return fail(KGX_EINVAL, "kgx_fa_parse_device: d_text is not aligned to 16 bytes");
    return fa_parse_device(c, static_cast<const uint8_t *>(d_text), n, flags, out);
}

int kgx_fa_parse(kgx_ctx *c, const char *text, uint64_t n, uint32_t flags, kgx_fa_seqs *out)
{
    if (int rc = parse_checks(c, text, n, flags, out))
        return rc;
    if (!n)
        return (flags & KGX_FA_FINISHED) ? fa_parse_device(c, nullptr, 0, flags, out) : KGX_OK;
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
    if (int rc = fa_parse_device(c, c->fp_text.as<uint8_t>(), n, flags, out))
        return rc;
    HIP_TRY(hipEventElapsedTime(&out->upload_ms, c->fp_events[0], c->fp_events[1]));
    return KGX_OK;
}

}  // extern "C"
