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
 * The scan over those maps is kgx_text_scan.h's, shared with the FASTA parser
 * (kgx_fa_parse.hip); this file gives it the machine:
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
#include "kgx_text_scan.h"

using namespace kgx;
using namespace kgx::text_scan;

namespace {

struct FqMachine {
    enum : uint32_t { S_START, S_ID, S_DEF, S_DATA, S_PLUS_START, S_PLUS, S_QUAL, N_STATES };
    enum : uint32_t { C_NL, C_AT, C_PLUS, C_BLANK, C_LETTER, C_OTHER, N_CLASSES };
    static constexpr uint32_t END_TAKES_BYTE = 1; /* a record ends with its quality line's newline */

    static constexpr uint32_t next_state(uint32_t s, uint32_t c)
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

    static constexpr uint32_t event_of(uint32_t s, uint32_t c)
    {
        switch (s) {
        case S_START: return c == C_AT ? 0 : EV_BAD;
        case S_ID: return (c == C_NL || c == C_BLANK) ? 0 : EV_ID;
        case S_DATA: return c == C_NL ? 0 : c == C_LETTER ? EV_DATA : EV_BAD;
        case S_PLUS_START: return c == C_PLUS ? 0 : EV_BAD;
        case S_QUAL: return c == C_NL ? EV_END : 0;
        default: return 0;
        }
    }

    static __device__ __forceinline__ uint32_t class_of(uint32_t b)
    {
        const bool letter = ((b | 0x20u) - 'a') < 26u;
        return b == '\n' ? C_NL
               : b == '@' ? C_AT
               : b == '+' ? C_PLUS
               : (b == ' ' || b == '\t') ? C_BLANK
               : letter ? C_LETTER
                        : C_OTHER;
    }

    /* kgx_fq_reads.error */
    static __device__ __forceinline__ uint32_t error_code(uint32_t s, uint32_t b)
    {
        return s == S_START ? (b == '>' ? 1u : 2u) : s == S_DATA ? 3u : 4u;
    }
};

/* 1. a tile's map */
__global__ __launch_bounds__(256) void fq_parse_map_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                           uint32_t *__restrict__ tile_map)
{
    map_body<FqMachine>(text, n, tile_map);
}

/* 2. one workgroup: every tile's entry state, and the text's end state in
 * tile_state[n_tiles] */
__global__ __launch_bounds__(256) void fq_parse_state_kernel(const uint32_t *__restrict__ tile_map, uint32_t n_tiles,
                                                             uint8_t *__restrict__ tile_state)
{
    state_body<FqMachine>(tile_map, n_tiles, tile_state);
}

/* 3. the lanes' entry states, the tile's counts, the first offending byte */
__global__ __launch_bounds__(256) void fq_parse_count_kernel(const uint8_t *__restrict__ text, uint64_t n,
                                                             const uint8_t *__restrict__ tile_state,
                                                             uint8_t *__restrict__ lane_state,
                                                             uint4 *__restrict__ tile_cnt, uint64_t *error_key)
{
    count_body<FqMachine>(text, n, tile_state, lane_state, tile_cnt, error_key);
}

/* 4. one workgroup: the exclusive sums of the tiles' counts (x ids, y bases,
 * z record ends, w newlines; n <= KGX_FQ_PARSE_MAX keeps them in 32 bits) and
 * the call's sums */
__global__ __launch_bounds__(256) void fq_parse_sums_kernel(const uint4 *__restrict__ tile_cnt, uint32_t n_tiles,
                                                            uint4 *__restrict__ tile_pre, uint64_t *sums)
{
    sums_body(tile_cnt, n_tiles, tile_pre, sums);
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
    write_body<FqMachine>(text, n, lane_state, tile_pre, n_records, n_ids, n_bases, error_pos, bases, read_offsets, ids,
                          id_offsets, sums);
}

/* 6. the records without an id */
__global__ __launch_bounds__(256) void fq_parse_no_id_kernel(const uint64_t *__restrict__ id_offsets, uint32_t n_records,
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
    c->fp_last = kgx_fq_reads{};
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
    const uint64_t n_ids = h[SUM_IDS], n_bases = h[SUM_DATA], n_rec = h[SUM_RECORDS], cut_newlines = h[SUM_NEWLINES];
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
    out->n_bases = tail ? n_bases : h[SUM_DATA_AT_END];
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
    c->fp_last = *out;
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
    if (!n) {
        c->fp_last = kgx_fq_reads{};
        return KGX_OK;
    }
    if (reinterpret_cast<uintptr_t>(d_text) & 15u)
        return fail(KGX_EINVAL, "kgx_fq_parse_device: d_text is not aligned to 16 bytes");
    return fq_parse_device(c, static_cast<const uint8_t *>(d_text), n, flags, out);
}

int kgx_fq_parse(kgx_ctx *c, const char *text, uint64_t n, uint32_t flags, kgx_fq_reads *out)
{
    if (int rc = parse_checks(c, text, n, flags, out))
        return rc;
    if (!n) {
        c->fp_last = kgx_fq_reads{};
        return KGX_OK;
    }
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
