/*
 * kgx_score.hip -- the scorers of the lookup path, the best call and the OTU
 * tallies, each over one sequence's hits in the tiled layout.
 *
 *   score  : the gather_hits / process_set_of_hits run state machine, one
 *            lane per sequence, O(1) state (no 40,000-entry buffer); the
 *            wave-parallel scorer for long sequences
 *
 * Reference behaviour restated (kguts.cc line numbers): run rules 734-781 and
 * 808-876.
 */
#include "kgx_device.h"
#include "kgx_lstd.h"

#include <type_traits>

namespace kgx {

/* ------------------------------------------------------------------------ */
/* hits of one sequence in the tiled layout                                  */
/* ------------------------------------------------------------------------ */

/*
 * Calls f(storage_start, count, ordinal0) for each run of the sequence's hits
 * (windows [gw0, gw1)): within one mask word, the sequence's hits are a
 * contiguous stretch of its tile's compacted hits.  Returns the hit count.
 */
template <class F>
__device__ __forceinline__ uint32_t for_each_run(const uint64_t *__restrict__ hit_mask,
                                                 uint32_t tile_windows, uint64_t gw0, uint64_t gw1,
                                                 F &&f)
{
    if (gw0 >= gw1)
        return 0;
    const uint32_t J = tile_windows / 64;
    const uint64_t gfirst = gw0 >> 6, glast = (gw1 - 1) >> 6;
    uint64_t tile = gfirst / J;
    uint32_t pre = 0; /* tile's hits before word g */
    for (uint64_t g = tile * J; g < gfirst; g++)
        pre += (uint32_t)__popcll(hit_mask[g]);
    uint32_t ordinal = 0;
    uint64_t next = hit_mask[gfirst];
    for (uint64_t g = gfirst; g <= glast; g++) {
        if (g != gfirst && g % J == 0) {
            tile = g / J;
            pre = 0;
        }
        const uint64_t full = next;
        if (g < glast)
            next = hit_mask[g + 1]; /* in flight while f works on word g */
        const uint32_t lo = g == gfirst ? (uint32_t)(gw0 & 63) : 0u;
        const uint32_t hi = g == glast ? (uint32_t)((gw1 - 1) & 63) + 1 : 64u;
        const uint64_t bits = full & bit_range(lo, hi);
        const uint32_t cnt = (uint32_t)__popcll(bits);
        if (cnt) /* the hits' positions: bit b of `bits` is position 64 g + b - gw0 */
            f(tile * tile_windows + pre + (uint32_t)__popcll(full & bit_range(0, lo)), cnt, ordinal, bits,
              (uint32_t)(64 * g - gw0));
        ordinal += cnt;
        pre += (uint32_t)__popcll(full);
    }
    return ordinal;
}

/*
 * The same walk for the lean scorer, whose caller knows that the batch's hit
 * slots (and so its windows) stay below 2^32: 32-bit indices, one running
 * slot index instead of tile and count, and the next mask word not loaded
 * ahead (it would hold two more registers across f).  Same arguments to f.
 */
template <class F>
__device__ __forceinline__ uint32_t for_each_run_lean(const uint64_t *__restrict__ hit_mask,
                                                      uint32_t tile_windows, uint32_t gw0, uint32_t gw1,
                                                      F &&f)
{
    if (gw0 >= gw1)
        return 0;
    const uint32_t J = tile_windows / 64;
    const uint32_t gfirst = gw0 >> 6, glast = (gw1 - 1) >> 6;
    uint32_t slot = gfirst / J * tile_windows; /* storage slot of the first hit of word g */
    for (uint32_t g = gfirst / J * J; g < gfirst; g++)
        slot += (uint32_t)__popcll(hit_mask[g]);
    uint32_t ordinal = 0;
    for (uint32_t g = gfirst; g <= glast; g++) {
        if (g != gfirst && g % J == 0)
            slot = g / J * tile_windows;
        const uint64_t full = hit_mask[g];
        const uint32_t lo = g == gfirst ? (gw0 & 63) : 0u;
        const uint32_t hi = g == glast ? ((gw1 - 1) & 63) + 1 : 64u;
        const uint64_t bits = full & bit_range(lo, hi);
        const uint32_t cnt = (uint32_t)__popcll(bits);
        if (cnt)
            f(slot + (uint32_t)__popcll(full & bit_range(0, lo)), cnt, ordinal, bits, 64 * g - gw0);
        ordinal += cnt;
        slot += (uint32_t)__popcll(full);
    }
    return ordinal;
}

/* ------------------------------------------------------------------------ */
/* score                                                                     */
/* ------------------------------------------------------------------------ */

/*
 * The run state machine of gather_hits (kguts.cc:808-876) and
 * process_set_of_hits (kguts.cc:734-781), one lane per sequence.  The
 * reference keeps up to 40000 hits in a buffer and rescans it at every flush;
 * here the buffer is summarised by O(1) state that yields the same call:
 *   n         number of buffered hits (capped at RUN_CAP, kguts.cc:850-851)
 *   cur       current_fI
 *   cnt/wsum  count and f32 sum (in append order) of buffered hits with
 *             fI == cur -- exactly the reference's flush loop
 *   first/last position of buffer[0] / of the last buffered hit with fI == cur
 *   p1, p2    the last two buffered hits (gap rule, order constraint,
 *             pair switch and carry-over read only these)
 * With OTU output requested, buffered hits are flagged KGX_HIT_IN_RUN (and
 * KGX_HIT_COUNTED when their function is their run's current_fI); each
 * emitted call records its run's ordinal hit range, and a second walk flags
 * the COUNTED hits inside emitted ranges KGX_HIT_OTU -- the hits the
 * reference tallies into otu_map (kguts.cc:760-768).
 */
struct RunTail {
    uint32_t pos, fI, idx;
    float wt;
    uint32_t avg;
    uint32_t fb; /* the record's flag dword without flags */
    uint64_t at; /* storage index */
};

constexpr int SCORE_BATCH = 8; /* records per load batch (double-buffered); 2 for short sequences */
constexpr int SCORE_LEAN_BATCH = 4; /* the same of the lean form */

/* The lean form reads of a record only dwords 1 and 2 (HitFields::fi and
 * ::wt, the same dwords in both hit formats) as one 8-byte load at a 4-byte
 * boundary; the general form reads the record whole. */
struct __attribute__((packed, aligned(4))) HitYZ {
    uint32_t y, z;
};
__device__ __forceinline__ uint2 load_yz(const uint4 *rec)
{
    const HitYZ v = *reinterpret_cast<const HitYZ *>(reinterpret_cast<const uint32_t *>(rec) + 1);
    return make_uint2(v.y, v.z);
}
__device__ __forceinline__ const uint4 &as_hit(const uint4 &r) { return r; }
__device__ __forceinline__ uint4 as_hit(const uint2 &r) { return make_uint4(0u, r.x, r.y, 0u); }

/*
 * LEAN: calls only, order_constraint 0 (launch_score's choice).  The fields
 * that only the OTU flags, the ranges and the order constraint read -- a
 * hit's ordinal, storage slot, flag dword and avg, run_start, last_idx -- are
 * then dead and the compiler drops them; the records in flight are (y, z)
 * pairs, and the mask words are walked by for_each_run_lean (32-bit indices,
 * no read-ahead).  The run rules below are written once for both forms; the
 * general form compiles to the instructions it had before the lean one was
 * split off (tools/asm_compare.py), which is why its record load and its
 * walker are spelled out beside the lean ones and not behind a common helper.
 * The function has two parts, the early-out test (EARLY), made from mask
 * words alone, and the runs (RUNS); score_lean_kernel calls them apart.
 * Returns false when the sequence left at the early-out (its counts are
 * written), true otherwise.
 */
template <bool PK, int SB = SCORE_BATCH, bool LEAN = false, bool EARLY = true, bool RUNS = true>
__device__ __forceinline__ bool score_sequence(
    uint32_t s, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, uint4 *__restrict__ hot, kgx_call *__restrict__ calls,
    uint2 *__restrict__ ranges, uint32_t *__restrict__ hit_count, uint32_t *__restrict__ call_count,
    const kgx_params &prm, uint32_t want)
{
    /* LEAN: launch_score has seen that the hit slots stay below 2^32 */
    typedef typename std::conditional<LEAN, uint32_t, uint64_t>::type Idx;
    const Idx gw0 = (Idx)wbase[s], gw1 = (Idx)wbase[s + 1];
    auto each_run = [&](auto &&f) {
        if constexpr (LEAN)
            return for_each_run_lean(hit_mask, tile_windows, gw0, gw1, f);
        else
            return for_each_run(hit_mask, tile_windows, gw0, gw1, f);
    };
    /* LEAN: launch_score sends only requests for calls without OTU output */
    const bool want_calls = LEAN || (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = !LEAN && (want & KGX_WANT_OTU) != 0;
    if (EARLY) {
        if (!want_calls && !want_otu) {
            /* process_set_of_hits returns before doing anything (kguts.cc:737) */
            hit_count[s] = each_run([](Idx, uint32_t, uint32_t, uint64_t, uint32_t) {});
            call_count[s] = 0;
            return false;
        }
        if (!want_otu && prm.min_hits > 0 && gw1 > gw0) {
            /* fewer hits than min_hits: no run can reach a call (a call counts
             * at most the sequence's hits, kguts.cc:757-770), and without OTU
             * output the run flags are not kept -- count and leave without
             * reading a record (fq fragments: ~16 windows, < 1 hit each) */
            uint32_t nh = 0;
            for (Idx g = gw0 >> 6; g <= (gw1 - 1) >> 6; g++) {
                const uint32_t lo = g == (gw0 >> 6) ? (uint32_t)(gw0 & 63) : 0u;
                const uint32_t hi = g == ((gw1 - 1) >> 6) ? (uint32_t)((gw1 - 1) & 63) + 1 : 64u;
                nh += (uint32_t)__popcll(hit_mask[g] & bit_range(lo, hi));
            }
            if ((int)nh < prm.min_hits) {
                hit_count[s] = nh;
                call_count[s] = 0;
                return false;
            }
        }
    }
    if (!RUNS)
        return true;
    typedef typename std::conditional<LEAN, uint2, uint4>::type Rec;

    typedef HitFields<PK> HF;
    constexpr uint32_t F_RUN = KGX_HIT_IN_RUN << HF::FLAG_SHIFT, F_CNT = KGX_HIT_COUNTED << HF::FLAG_SHIFT,
                       F_OTU = KGX_HIT_OTU << HF::FLAG_SHIFT;
    constexpr int FD = HF::FLAG_DWORD;
    uint32_t *hw = reinterpret_cast<uint32_t *>(hot); /* 4 dwords per hit, flags in dword FD */
    const Idx cbase = gw0; /* calls / ranges of s live at [gw0, ...) */
    const uint32_t gap = (uint32_t)prm.max_gap;
    int n = 0;
    uint32_t cur = 0, first_pos = 0, last_pos = 0, last_idx = 0, run_start = 0;
    int cnt = 0;
    float wsum = 0.0f;
    RunTail p1 = {0, 0, 0, 0.0f, 0, 0, 0}, p2 = {0, 0, 0, 0.0f, 0, 0, 0};
    uint32_t ncalls = 0;

    auto flush = [&]() {
        if (n == 0)
            return; /* min_hits <= 0 final flush: reference UB, emit nothing */
        if (cnt >= prm.min_hits && wsum >= (float)prm.min_weighted_hits) {
            if (want_calls) {
                kgx_call cl;
                cl.start = first_pos;
                cl.end = last_pos + (KMER - 1);
                cl.count = cnt;
                cl.function_index = cur;
                cl.weighted_hits = wsum;
                calls[cbase + ncalls] = cl;
            }
            if (want_otu)
                ranges[cbase + ncalls] = make_uint2(run_start, last_idx);
            ncalls++;
        }
        if (n >= 2 && p2.fI != cur && p2.fI == p1.fI) { /* carry the pair */
            cur = p1.fI;
            n = 2;
            run_start = p2.idx;
            first_pos = p2.pos;
            cnt = 2;
            wsum = 0.0f + p2.wt;
            wsum = wsum + p1.wt;
            last_pos = p1.pos;
            last_idx = p1.idx;
            if (want_otu) {
                hw[4 * p2.at + FD] = p2.fb | F_RUN | F_CNT;
                hw[4 * p1.at + FD] = p1.fb | F_RUN | F_CNT;
            }
        } else {
            n = 0;
        }
    };

    auto step = [&](const Rec &rec, uint32_t i, Idx at, uint32_t pos) {
        const auto &r = as_hit(rec);
        const uint32_t avg = HF::avg(r);
        const uint32_t fI = HF::fi(r);
        const float wt = __uint_as_float(HF::wt(r));
        const uint32_t fb = HF::flag_base(r);
        /* gap rule (kguts.cc:821-831), unsigned arithmetic */
        if (n > 0 && p1.pos + gap < pos) {
            if (n >= prm.min_hits)
                flush();
            else
                n = 0;
        }
        if (n == 0) {
            cur = fI;
            cnt = 0;
            wsum = 0.0f;
            run_start = i;
            first_pos = pos;
        }
        bool accept = true;
        if (!LEAN && prm.order_constraint && n > 0) { /* kguts.cc:838-842 */
            const uint32_t d = (pos - p1.pos) - (uint32_t)((int)p1.avg - (int)avg);
            accept = (fI == p1.fI) && d <= 20u;
        }
        if (accept) {
            if (n < RUN_CAP) {
                n++;
                const bool counted = fI == cur;
                if (want_otu) /* flags only feed the OTU pass */
                    hw[4 * at + FD] = fb | F_RUN | (counted ? F_CNT : 0u);
                if (counted) {
                    cnt++;
                    wsum += wt;
                    last_pos = pos;
                    last_idx = i;
                }
                p2 = p1;
                p1 = RunTail{pos, fI, i, wt, avg, fb, at};
            }
            /* pair switch (kguts.cc:852-856) */
            if (n > 1 && cur != fI && p2.fI == p1.fI)
                flush();
        }
    };

    /* hits are read SB at a time and double-buffered: batch b+1's
     * loads are in flight while batch b runs through the state machine (the
     * machine is serial, its inputs are not) */
    auto load_batch = [&](Rec *rb, Idx at0, uint32_t b, uint32_t c) {
#pragma unroll
        for (int k = 0; k < SB; k++)
            if (b + k < c) {
                if constexpr (LEAN)
                    rb[k] = load_yz(hot + (at0 + b + k));
                else
                    rb[k] = hot[at0 + b + k];
            }
    };
    const uint32_t nh = each_run(
                                     [&](Idx at0, uint32_t c, uint32_t ord0, uint64_t bits, uint32_t pbase) {
        Rec ra[SB], rb[SB];
        load_batch(ra, at0, 0, c);
        for (uint32_t b = 0; b < c; b += 2 * SB) {
            if (b + SB < c)
                load_batch(rb, at0, b + SB, c);
#pragma unroll
            for (int k = 0; k < SB; k++)
                if (b + k < c) {
                    step(ra[k], ord0 + b + k, at0 + b + k, pbase + (uint32_t)__builtin_ctzll(bits));
                    bits &= bits - 1;
                }
            if (b + SB >= c)
                break;
            if (b + 2 * SB < c)
                load_batch(ra, at0, b + 2 * SB, c);
#pragma unroll
            for (int k = 0; k < SB; k++)
                if (b + SB + k < c) {
                    step(rb[k], ord0 + b + SB + k, at0 + b + SB + k,
                         pbase + (uint32_t)__builtin_ctzll(bits));
                    bits &= bits - 1;
                }
        }
    });
    if (n >= prm.min_hits) /* kguts.cc:873-876 */
        flush();
    hit_count[s] = nh;
    call_count[s] = want_calls ? ncalls : 0;

    /* OTU flags: COUNTED hits inside an emitted call's ordinal range (ranges
     * are disjoint and in order) */
    if (want_otu && ncalls > 0) {
        uint32_t ci = 0;
        uint2 rg = ranges[cbase];
        const uint32_t end = ranges[cbase + ncalls - 1].y;
        for_each_run(hit_mask, tile_windows, gw0, gw1,
                     [&](Idx at0, uint32_t c, uint32_t ord0, uint64_t, uint32_t) {
            for (uint32_t k = 0; k < c; k++) {
                const uint32_t i = ord0 + k;
                if (i > end)
                    return;
                while (i > rg.y) /* i <= end keeps ci < ncalls */
                    rg = ranges[cbase + ++ci];
                if (i >= rg.x) {
                    const uint32_t f = hw[4 * (at0 + k) + FD];
                    if (f & F_CNT)
                        hw[4 * (at0 + k) + FD] = f | F_OTU;
                }
            }
        });
    }
    return true;
}

/* skip_above: sequences with windows in (skip_above, RUN_CAP] are the wave
 * scorer's (hybrid dispatch); ~0u = none */
template <bool PK, int SB>
__global__ __launch_bounds__(256) void score_kernel(
    uint32_t n_seq, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, uint4 *__restrict__ hot, kgx_call *__restrict__ calls,
    uint2 *__restrict__ ranges, uint32_t *__restrict__ hit_count, uint32_t *__restrict__ call_count,
    kgx_params prm, uint32_t want, uint32_t skip_above)
{
    /* grid-stride: a capped grid (KGX_SCORE_GRID_CAP) walks several
     * sequences per lane */
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_seq; s += gridDim.x * blockDim.x) {
        const uint64_t w = wbase[s + 1] - wbase[s];
        if (w > skip_above && w <= (uint64_t)RUN_CAP)
            continue;
        score_sequence<PK, SB>(s, wbase, hit_mask, tile_windows, hot, calls, ranges, hit_count, call_count, prm,
                               want);
    }
}

/*
 * The lean lane scorer (score_sequence<.., LEAN>: calls without OTU output,
 * order_constraint 0), one workgroup per 256 sequences.  Every lane makes the
 * early-out test for its own sequence from the mask words.  PACK: the
 * sequences that stay are then listed in LDS in block order -- a ballot and
 * lanes_below per wave, four wave totals -- and after one barrier lane i
 * scores the i-th of them, so the lanes that work fill whole waves and a wave
 * left with nothing returns its registers at once.  Each sequence's results
 * go to its own slots as in score_kernel.  When every lane stays (min_hits
 * <= 0) lane i finds its own sequence again: the packing costs the barrier.
 */
template <bool PK, int SB, bool PACK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void score_lean_kernel(
    uint32_t n_seq, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, uint4 *__restrict__ hot, kgx_call *__restrict__ calls,
    uint32_t *__restrict__ hit_count, uint32_t *__restrict__ call_count, kgx_params prm, uint32_t want,
    uint32_t skip_above)
{
    __shared__ uint32_t stay_seq[4][64]; /* per wave: its staying sequences, in lane order */
    __shared__ uint32_t stay_n[4];
    /* grid-stride by workgroup (KGX_SCORE_GRID_CAP), uniform over the workgroup */
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < n_seq; base += (uint64_t)gridDim.x * 256u) {
        uint32_t s = (uint32_t)min(base + threadIdx.x, (uint64_t)n_seq);
        bool stay = false;
        if (s < n_seq) {
            const uint64_t w = wbase[s + 1] - wbase[s];
            stay = !(w > skip_above && w <= (uint64_t)RUN_CAP) &&
                   score_sequence<PK, SB, true, true, false>(s, wbase, hit_mask, tile_windows, hot, calls, nullptr,
                                                             hit_count, call_count, prm, want);
        }
        if constexpr (PACK) {
            const uint32_t wave = threadIdx.x >> 6;
            const uint64_t m = __ballot(stay);
            if (stay)
                stay_seq[wave][lanes_below(m)] = s;
            if (lane_id() == 0)
                stay_n[wave] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t i = threadIdx.x, w = 0;
            while (w < 4 && i >= stay_n[w])
                i -= stay_n[w++];
            stay = w < 4;
            if (stay)
                s = stay_seq[w][i];
        }
        if (stay)
            score_sequence<PK, SB, true, false, true>(s, wbase, hit_mask, tile_windows, hot, calls, nullptr, hit_count,
                                                call_count, prm, want);
        if constexpr (PACK)
            if (base + (uint64_t)gridDim.x * 256u < n_seq)
                __syncthreads(); /* the lists are rewritten by the next round */
    }
}

/* ------------------------------------------------------------------------ */
/* score, wave-parallel                                                      */
/* ------------------------------------------------------------------------ */

/*
 * The same run rules (gather_hits kguts.cc:808-876, process_set_of_hits
 * kguts.cc:734-781) evaluated 64 hits at a time by one wave, for
 * order_constraint == 0 and sequences of at most RUN_CAP windows (every hit is
 * then buffered: the 40,000-entry cap never binds).  Under those conditions
 * the state machine reduces to per-hit predicates over a hit and its
 * predecessor in the same sequence:
 *   brk[i]  = first hit of its sequence, or prev.pos + max_gap < pos
 *             (unsigned, kguts.cc:821-831): a new run starts at i;
 *   mark[i] = brk[i] or fI[i] == fI[i-1]: after hit i, current_fI = fI[i];
 *   cur[i]  = fI of the last marked hit at or before i (a segmented scan:
 *             one ballot and a highest-set-bit per lane);
 *   switch  = fI[i] == fI[i-1] != cur[i-1] (kguts.cc:852-856): the run so far
 *             is flushed and the carried pair i-1, i starts a new sub-run
 *             (kguts.cc:771-779; a gap flush never carries: its last two hits
 *             would have switched already).
 * Sub-runs start at brk hits and one hit before switch hits; a sub-run's call
 * counts its hits with fI == its current_fI (its first hit always does), from
 * its first hit to the last such hit, and is emitted when count >= min_hits
 * and the f32 sum of their weights, added in hit order from 0.0f, is >=
 * min_weighted_hits -- the same condition at a gap, a switch and the final
 * flush.  Everything but that sum is ballots, bit counts and shuffles; the
 * sums run serially (v_readlane + v_add_f32 in hit order) only over sub-runs
 * that reach min_hits.
 *
 * Work: wave w takes the sequences whose first window lies in windows
 * [w R, (w+1) R) (R = SCORE_WAVE_TILES tiles; found from tile_seq), walks
 * their hit-mask words (64 at a time in a register) and queues each hit's
 * (position, sequence, first window, storage slot) in LDS; every 64 queued
 * hits -- of one long sequence or of many short fragments -- are one chunk.
 * The open sub-run, the last hit and the open sequence's call count carry
 * from chunk to chunk.  A sub-run that spans chunks and is emitted gets its
 * OTU flags by a walk over its windows.  Sequences longer than RUN_CAP
 * windows run the serial machine (score_sequence) on one lane.
 */
constexpr uint32_t SQ = 256; /* queue entries per wave: a chunk in flight, the next, a word's overflow */

struct ScoreQueue {
    uint32_t pos[SQ];
    uint32_t seq[SQ];
    uint32_t at[SQ];
    uint64_t mw[64]; /* hit-mask words gb .. gb + 63 */
    uint64_t wb[65]; /* window bases of sequences sb .. sb + 64 */
};


/* first sequence whose first window is >= x (x a tile boundary below the
 * batch's window count); tile_seq[x / T] owns window x */
__device__ __forceinline__ uint32_t seq_lower_bound(const uint64_t *__restrict__ wbase,
                                                    const uint32_t *__restrict__ tile_seq, uint32_t T, uint64_t x)
{
    uint32_t s = tile_seq[x / T];
    if (wbase[s] < x)
        return s + 1;
    while (s > 0 && wbase[s - 1] == x) /* empty sequences right before it */
        s--;
    return s;
}

template <bool PK>
__global__ __launch_bounds__(256) void score_wave_kernel(
    uint32_t n_seq, const uint64_t *__restrict__ wbase, const uint32_t *__restrict__ tile_seq,
    const uint64_t *__restrict__ hit_mask, uint32_t tile_windows, uint32_t wave_tiles, uint4 *__restrict__ hot,
    kgx_call *__restrict__ calls, uint32_t *__restrict__ hit_count, uint32_t *__restrict__ call_count,
    kgx_params prm, uint32_t want, uint32_t only_above, const uint32_t *__restrict__ plan_status)
{
    /* hybrid dispatch: only sequences over only_above windows are this
     * kernel's; the plan's longest-sequence word says whether there are any */
    if (only_above && plan_status[1] <= only_above)
        return;
    __shared__ ScoreQueue queues[4];
    typedef HitFields<PK> HF;
    constexpr uint32_t F_RUN = KGX_HIT_IN_RUN << HF::FLAG_SHIFT, F_CNT = KGX_HIT_COUNTED << HF::FLAG_SHIFT,
                       F_OTU = KGX_HIT_OTU << HF::FLAG_SHIFT;
    constexpr int FD = HF::FLAG_DWORD;
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    ScoreQueue &Q = queues[threadIdx.x >> 6];
    uint32_t *hw = reinterpret_cast<uint32_t *>(hot);
    const uint32_t lane = lane_id();
    const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t R = (uint64_t)tile_windows * wave_tiles;
    const uint64_t W = wbase[n_seq];
    const uint64_t x0 = (uint64_t)w * R;
    if (w > 0 && x0 >= W)
        return;
    const uint32_t s_lo = w == 0 ? 0u : seq_lower_bound(wbase, tile_seq, tile_windows, x0);
    const uint32_t s_hi = x0 + R >= W ? n_seq : seq_lower_bound(wbase, tile_seq, tile_windows, x0 + R);
    const bool want_calls = (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = (want & KGX_WANT_OTU) != 0;
    const bool scoring = want_calls || want_otu;
    const uint32_t J = tile_windows / 64;
    const uint32_t gap = (uint32_t)prm.max_gap;
    const float min_wh = (float)prm.min_weighted_hits;

    /* ---- the open sub-run (O) and the last hit, carried across chunks ---- */
    bool o_valid = false, o_span = false;
    uint32_t o_seq = NONE, o_cur = 0, o_cnt = 0, o_first = 0, o_last = 0, o_ncalls = 0;
    float o_wsum = 0.0f;
    uint32_t p_pos = 0, p_fi = 0, p_fb = 0, p_at = 0;
    float p_wt = 0.0f;

    /* OTU flags of an emitted sub-run that spans chunks: its hits are the
     * sequence's hits in windows [first, last]; the ones with fI == cur count */
    auto otu_fixup = [&](uint64_t gw0, uint32_t first, uint32_t last, uint32_t cur) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); /* earlier flag stores are done */
        const uint64_t a = gw0 + first, b = gw0 + last;
        for (uint64_t g = a >> 6; g <= (b >> 6); g++) {
            const uint64_t full = hit_mask[g];
            const uint32_t lo = g == (a >> 6) ? (uint32_t)(a & 63) : 0u;
            const uint32_t hi = g == (b >> 6) ? (uint32_t)(b & 63) + 1 : 64u;
            const uint64_t bits = full & bit_range(lo, hi);
            const uint64_t tile = g / J;
            uint32_t pre = 0;
            for (uint64_t q = tile * J; q < g; q++)
                pre += (uint32_t)__popcll(hit_mask[q]);
            if ((bits >> lane) & 1) {
                const uint64_t at = tile * tile_windows + pre + lanes_below(full);
                const uint4 r = hot[at];
                if (HF::fi(r) == cur)
                    hw[4 * at + FD] = HF::flag_base(r) | F_RUN | F_CNT | F_OTU;
            }
        }
    };
    /* flush of O: the call (kguts.cc:757-770) when count and weight reach the minimums */
    auto close_open = [&]() -> bool {
        const bool em = (int)o_cnt >= prm.min_hits && o_wsum >= min_wh;
        if (em) {
            const uint64_t gw0 = wbase[o_seq];
            if (want_calls && lane == 0) {
                kgx_call cl;
                cl.start = o_first;
                cl.end = o_last + (KMER - 1);
                cl.count = (int32_t)o_cnt;
                cl.function_index = o_cur;
                cl.weighted_hits = o_wsum;
                calls[gw0 + o_ncalls] = cl;
            }
            o_ncalls++;
            if (want_otu && o_span)
                otu_fixup(gw0, o_first, o_last, o_cur);
        }
        return em;
    };

    uint32_t qhead = 0, qissue = 0, qtail = 0;

    /* one chunk: queue entries [qhead, qhead + n), n <= 64, records in r */
    auto process_chunk = [&](uint32_t n, const uint4 &r) {
        const uint32_t k = lane;
        const bool act = k < n;
        const uint64_t ACT = n >= 64 ? ~0ull : ((1ull << n) - 1);
        const uint32_t e = (qhead + k) & (SQ - 1);
        const uint32_t pos = act ? Q.pos[e] : 0u;
        const uint32_t seq = act ? Q.seq[e] : NONE;
        const uint32_t at = act ? Q.at[e] : 0u;
        const uint32_t fi = HF::fi(r);
        const float wt = __uint_as_float(HF::wt(r));
        const uint32_t fb = HF::flag_base(r);

        /* the predecessor of each hit (lane 0: the carried last hit) */
        uint32_t ppos = __shfl_up(pos, 1), pfi = __shfl_up(fi, 1), pseq = __shfl_up(seq, 1);
        if (k == 0) {
            ppos = p_pos;
            pfi = p_fi;
            pseq = o_valid ? o_seq : NONE;
        }
        const bool newseq = seq != pseq;
        const bool brk = newseq || (ppos + gap < pos);
        const bool eqp = !brk && fi == pfi;
        const uint64_t M = __ballot(act && (brk || eqp));
        const int jm = hibit(M & lanes_le(k));
        uint32_t cur = __shfl(fi, jm < 0 ? 0 : jm);
        if (jm < 0)
            cur = o_cur;
        uint32_t pcur = __shfl_up(cur, 1);
        if (k == 0)
            pcur = o_cur;
        const bool sw = act && eqp && fi != pcur;
        const uint64_t SW = __ballot(sw), NS = __ballot(act && newseq);
        const uint64_t S = (__ballot(act && brk) | (SW >> 1)) & ACT; /* sub-run starts */
        const bool memb = act && (fi == cur || ((S >> k) & 1));
        const uint64_t MEMB = __ballot(memb);

        /* a switch at lane 0: O is flushed before this chunk and the pair
         * (last hit, lane 0) starts the new O */
        if (SW & 1) {
            close_open();
            if (want_otu && lane == 0)
                hw[4 * (uint64_t)p_at + FD] = p_fb | F_RUN | F_CNT;
            o_cur = rl32(fi, 0);
            o_cnt = 1;
            o_wsum = 0.0f + p_wt;
            o_first = p_pos;
            o_last = p_pos;
            o_span = true;
        }
        /* lanes before the first start continue O */
        const uint32_t fs = S ? lowbit(S) : n;
        if (fs > 0) {
            uint64_t mm = MEMB & bit_range(0, fs);
            o_cnt += (uint32_t)__popcll(mm);
            if (mm)
                o_last = rl32(pos, (uint32_t)hibit(mm));
            while (mm) {
                o_wsum = o_wsum + rlf(wt, lowbit(mm));
                mm &= mm - 1;
            }
        }
        bool o_emitted = false;
        if (fs < n && o_valid) {
            o_emitted = close_open();
            if (fs == 0 && (NS & 1)) /* O's sequence ended in the previous chunk */
                if (lane == 0)
                    call_count[o_seq] = want_calls ? o_ncalls : 0u;
        }

        /* sub-runs that start in this chunk, one per start lane */
        const bool is_start = (S >> k) & 1;
        const uint64_t above = S & ~lanes_le(k);
        const uint32_t e_k = above ? lowbit(above) : n;
        const uint64_t msg = MEMB & bit_range(k, e_k);
        const uint32_t c_seg = (uint32_t)__popcll(msg);
        const int lm = hibit(msg);
        const uint32_t last_pos = __shfl(pos, lm < 0 ? 0 : lm);
        const bool closed = e_k < n;
        const int b_open = hibit(S); /* the sub-run left open at the chunk's end */
        /* the f32 sums, serially, for the sub-runs that can be emitted and the open one */
        uint64_t SUM = __ballot(is_start && closed && (int)c_seg >= prm.min_hits);
        if (b_open >= 0)
            SUM |= 1ull << b_open;
        float ws = 0.0f;
        while (SUM) {
            const uint32_t b = lowbit(SUM);
            SUM &= SUM - 1;
            const uint64_t ab = S & ~lanes_le(b);
            uint64_t mm = MEMB & bit_range(b, ab ? lowbit(ab) : n);
            float acc = 0.0f;
            while (mm) {
                acc = acc + rlf(wt, lowbit(mm));
                mm &= mm - 1;
            }
            if (lane == b)
                ws = acc;
        }
        const uint64_t EMIT = __ballot(is_start && closed && (int)c_seg >= prm.min_hits && ws >= min_wh);
        /* call index: the calls of the lane's sequence before it (O's sequence
         * continues through the lanes before the chunk's first new sequence) */
        const int fsq = hibit(NS & lanes_le(k));
        const uint32_t from = fsq < 0 ? 0u : (uint32_t)fsq;
        const uint32_t idx = (fsq < 0 ? o_ncalls : 0u) + (uint32_t)__popcll(EMIT & bit_range(from, k));
        if (want_calls && ((EMIT >> k) & 1)) {
            kgx_call cl;
            cl.start = pos;
            cl.end = last_pos + (KMER - 1);
            cl.count = (int32_t)c_seg;
            cl.function_index = fi;
            cl.weighted_hits = ws;
            calls[wbase[seq] + idx] = cl;
        }
        /* sequences whose last hit is in this chunk (not its last lane) */
        if (act && k + 1 < n && ((NS >> (k + 1)) & 1))
            call_count[seq] = want_calls ? idx + (uint32_t)((EMIT >> k) & 1) : 0u;
        if (want_otu && act) {
            const int bk = hibit(S & lanes_le(k));
            const bool em = bk >= 0 ? ((EMIT >> bk) & 1) != 0 : o_emitted;
            hw[4 * (uint64_t)at + FD] = fb | F_RUN | (memb ? F_CNT : 0u) | (memb && em ? F_OTU : 0u);
        }

        /* carry */
        if (b_open >= 0) {
            const uint32_t b = (uint32_t)b_open;
            o_valid = true;
            o_seq = rl32(seq, b);
            o_cur = rl32(fi, b);
            o_cnt = rl32(c_seg, b);
            o_wsum = rlf(ws, b);
            o_first = rl32(pos, b);
            o_last = rl32(last_pos, b);
            o_ncalls = rl32(idx, b);
        }
        o_span = true;
        const uint32_t l = n - 1;
        p_pos = rl32(pos, l);
        p_fi = rl32(fi, l);
        p_wt = rlf(wt, l);
        p_fb = rl32(fb, l);
        p_at = rl32(at, l);
        qhead += n;
    };

    /* records of the queued chunk in flight while the previous one is scored */
    uint4 rpend = make_uint4(0, 0, 0, 0);
    uint32_t npend = 0;
    auto issue = [&](uint32_t n_new) { /* entries [qissue, qissue + n_new) */
        wave_lds_sync();
        uint4 r = make_uint4(0, 0, 0, 0);
        if (lane < n_new)
            r = hot[Q.at[(qissue + lane) & (SQ - 1)]];
        if (npend)
            process_chunk(npend, rpend);
        rpend = r;
        npend = n_new;
        qissue += n_new;
        wave_lds_sync();
    };

    /* ---- walk the wave's sequences and their hit-mask words ---- */
    uint32_t sb = NONE; /* Q.wb[j] = wbase[sb + j] */
    uint32_t hb = s_lo; /* lane j: hit count of sequence hb + j */
    uint32_t vhc = 0;
    uint64_t gb = ~0ull; /* Q.mw[j] = hit_mask[gb + j] */
    uint64_t pg = ~0ull, pfull = 0;
    uint32_t ppre = 0;
    auto flush_counts = [&](uint32_t upto) { /* sequences [hb, upto) */
        if (lane < upto - hb && vhc != NONE) {
            hit_count[hb + lane] = vhc;
            if (vhc == 0 || !scoring)
                call_count[hb + lane] = 0;
        }
    };
    for (uint32_t s = s_lo; s < s_hi; s++) {
        if (s - hb > 63) {
            flush_counts(s);
            hb = s;
            vhc = 0;
        }
        if (sb == NONE || s + 1 - sb > 64) {
            wave_lds_sync();
            sb = s;
            Q.wb[lane] = wbase[min(sb + lane, n_seq)];
            if (lane == 0)
                Q.wb[64] = wbase[min(sb + 64, n_seq)];
            wave_lds_sync();
        }
        const uint64_t gw0 = uni64(Q.wb[s - sb]), gw1 = uni64(Q.wb[s + 1 - sb]);
        if (gw1 - gw0 > (uint64_t)RUN_CAP || (only_above && gw1 - gw0 <= only_above)) {
            /* score_long_kernel's / (hybrid) the lane scorer's */
            if (lane == s - hb)
                vhc = NONE;
            continue;
        }
        uint32_t nh = 0;
        if (gw0 < gw1) {
            const uint64_t g0 = gw0 >> 6, g1 = (gw1 - 1) >> 6;
            for (uint64_t g = g0; g <= g1; g++) {
                if (gb == ~0ull || g - gb > 63) {
                    wave_lds_sync();
                    gb = g;
                    Q.mw[lane] = (gb + lane) * 64 < W ? hit_mask[gb + lane] : 0ull;
                    wave_lds_sync();
                }
                const uint64_t full = uni64(Q.mw[g - gb]);
                if (g != pg) { /* hits of g's tile before word g */
                    if (pg != ~0ull && g == pg + 1)
                        ppre = g % J == 0 ? 0u : ppre + (uint32_t)__popcll(pfull);
                    else {
                        ppre = 0;
                        for (uint64_t q = (g / J) * J; q < g; q++)
                            ppre += (uint32_t)__popcll(hit_mask[q]);
                    }
                    pg = g;
                    pfull = full;
                }
                const uint32_t lo = g == g0 ? (uint32_t)(gw0 & 63) : 0u;
                const uint32_t hi = g == g1 ? (uint32_t)((gw1 - 1) & 63) + 1 : 64u;
                const uint64_t bits = full & bit_range(lo, hi);
                if (!bits)
                    continue;
                const uint32_t c = (uint32_t)__popcll(bits);
                nh += c;
                if (!scoring)
                    continue;
                if ((bits >> lane) & 1) {
                    const uint32_t slot = (qtail + lanes_below(bits)) & (SQ - 1);
                    Q.pos[slot] = (uint32_t)(64 * g + lane - gw0);
                    Q.seq[slot] = s;
                    Q.at[slot] = (uint32_t)((g / J) * tile_windows + ppre + lanes_below(full));
                }
                qtail += c;
                if (qtail - qissue >= 64)
                    issue(64);
            }
        }
        if (lane == s - hb)
            vhc = nh;
    }
    flush_counts(s_hi);
    if (!scoring)
        return;
    if (qtail != qissue)
        issue(qtail - qissue);
    if (npend) {
        wave_lds_sync();
        process_chunk(npend, rpend);
    }
    if (o_valid) {
        close_open();
        if (lane == 0)
            call_count[o_seq] = want_calls ? o_ncalls : 0u;
    }
}

/* the sequences past RUN_CAP windows (the wave kernel leaves them): the
 * lane machine, which keeps the reference's 40,000-hit cap */
template <bool PK>
__global__ __launch_bounds__(256) void score_long_kernel(
    uint32_t n_seq, const uint64_t *__restrict__ wbase, const uint64_t *__restrict__ hit_mask,
    uint32_t tile_windows, uint4 *__restrict__ hot, kgx_call *__restrict__ calls,
    uint2 *__restrict__ ranges, uint32_t *__restrict__ hit_count, uint32_t *__restrict__ call_count,
    kgx_params prm, uint32_t want)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_seq && wbase[s + 1] - wbase[s] > (uint64_t)RUN_CAP)
        score_sequence<PK>(s, wbase, hit_mask, tile_windows, hot, calls, ranges, hit_count, call_count, prm, want);
}

hipError_t launch_score(uint32_t n_seq, uint64_t n_residues, const uint64_t *wbase, const uint32_t *tile_seq,
                        uint64_t max_tiles, const uint64_t *hit_mask, uint32_t tile_windows, uint4 *hot,
                        kgx_call *calls, void *ranges, uint32_t *hit_count, uint32_t *call_count,
                        kgx_params params, uint32_t want, uint32_t hit_format, int variant, uint32_t wave_tiles,
                        int lean, const uint32_t *plan_status, hipStream_t stream, bool *lean_taken)
{
    if (lean_taken)
        *lean_taken = false;
    if (n_seq == 0)
        return hipSuccess;
    const bool pk = hit_format == HIT_PACKED16;
    const dim3 lanes((n_seq + 255) / 256);
    /* the wave scorer: order_constraint 0, hit slots in 32 bits */
    const bool wave_ok = !params.order_constraint && max_tiles * tile_windows < (1ull << 32);
    wave_tiles = std::max<uint32_t>(1, wave_tiles);
    const uint64_t waves = std::max<uint64_t>(1, (max_tiles + wave_tiles - 1) / wave_tiles);
    const dim3 wgrid((uint32_t)((waves + 3) / 4));
#define KGX_WAVE(P, ABOVE)                                                                                      \
    hipLaunchKernelGGL(score_wave_kernel<P>, wgrid, dim3(256), 0, stream, n_seq, wbase, tile_seq, hit_mask,     \
                       tile_windows, wave_tiles, hot, calls, hit_count, call_count, params, want, (ABOVE), plan_status)
    if (variant == SCORE_WAVE_ONLY && wave_ok) { /* the caller knows no sequence exceeds RUN_CAP windows */
        if (pk)
            KGX_WAVE(true, 0u);
        else
            KGX_WAVE(false, 0u);
        return hipGetLastError();
    }
    if ((variant == SCORE_WAVE || variant == SCORE_WAVE_ONLY) && wave_ok) { /* every sequence up to RUN_CAP windows */
        if (pk) {
            KGX_WAVE(true, 0u);
            hipLaunchKernelGGL(score_long_kernel<true>, lanes, dim3(256), 0, stream, n_seq, wbase, hit_mask,
                               tile_windows, hot, calls, static_cast<uint2 *>(ranges), hit_count, call_count, params,
                               want);
        } else {
            KGX_WAVE(false, 0u);
            hipLaunchKernelGGL(score_long_kernel<false>, lanes, dim3(256), 0, stream, n_seq, wbase, hit_mask,
                               tile_windows, hot, calls, static_cast<uint2 *>(ranges), hit_count, call_count, params,
                               want);
        }
        return hipGetLastError();
    }
    /* the lane machine; in the hybrid (the default) sequences of (LONG_SEQ,
     * RUN_CAP] windows go to the wave scorer instead: one lane walking a
     * 30k-aa protein's hits would hold the whole stage for milliseconds */
    const bool hybrid = variant == SCORE_HYBRID && wave_ok;
    const uint32_t skip = hybrid ? LONG_SEQ : ~0u;
    /* short sequences (fq fragments: ~16 windows, <1 hit each) take the
     * 2-record batches: fewer registers, more waves to hide the loads of
     * sequences that mostly have no hits */
    const bool small = n_residues < 64ull * n_seq;
    /* KGX_SCORE_GRID_CAP (experiments): at most this many workgroups, each
     * lane walking several sequences, so the scorer holds fewer wave slots
     * beside the next batch's probe */
    static const uint32_t grid_cap = [] {
        const char *e = std::getenv("KGX_SCORE_GRID_CAP");
        return e ? (uint32_t)std::max(0L, std::strtol(e, nullptr, 10)) : 0u;
    }();
    const dim3 sgrid(grid_cap ? std::min<uint32_t>(lanes.x, grid_cap) : lanes.x);
#define KGX_SCORE(P, B)                                                                                          \
    hipLaunchKernelGGL((score_kernel<P, B>), sgrid, dim3(256), 0, stream, n_seq, wbase, hit_mask, tile_windows, hot, \
                       calls, static_cast<uint2 *>(ranges), hit_count, call_count, params, want, skip)
    /* option score_lean: calls without OTU output under order_constraint 0
     * (lookup_request's find_best_match) take the lean kernel, 1 = as it is,
     * 2 = with its working lanes packed; everything else the general one */
#define KGX_LEAN(P, B, PACK)                                                                                     \
    hipLaunchKernelGGL((score_lean_kernel<P, B, PACK>), sgrid, dim3(256), 0, stream, n_seq, wbase, hit_mask,     \
                       tile_windows, hot, calls, hit_count, call_count, params, want, skip)
#define KGX_LANES(P, B, LB)                                                                                       \
    do {                                                                                                         \
        if (lean_ok && lean >= 2)                                                                                \
            KGX_LEAN(P, LB, true);                                                                               \
        else if (lean_ok)                                                                                        \
            KGX_LEAN(P, LB, false);                                                                              \
        else                                                                                                     \
            KGX_SCORE(P, B);                                                                                     \
    } while (0)
    const bool lean_ok = lean > 0 && (want & KGX_WANT_CALLS) && !(want & KGX_WANT_OTU) && params.order_constraint == 0 &&
                         max_tiles * tile_windows < (1ull << 32); /* its slot indices are 32-bit */
    if (lean_taken)
        *lean_taken = lean_ok;
    if (pk && small)
        KGX_LANES(true, 2, 2);
    else if (pk)
        KGX_LANES(true, SCORE_BATCH, SCORE_LEAN_BATCH);
    else if (small)
        KGX_LANES(false, 2, 2);
    else
        KGX_LANES(false, SCORE_BATCH, SCORE_LEAN_BATCH);
#undef KGX_LANES
#undef KGX_LEAN
#undef KGX_SCORE
    if (hybrid) {
        if (pk)
            KGX_WAVE(true, LONG_SEQ);
        else
            KGX_WAVE(false, LONG_SEQ);
    }
#undef KGX_WAVE
    return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* best call: find_best_call (kguts.cc:1008-1199), one lane per sequence     */
/* (best_call_decide, kgx_lstd.h; the sequence's calls are rewritten in its */
/* own stretch of the workspace)                                            */
/* ------------------------------------------------------------------------ */
__global__ __launch_bounds__(256) void best_call_kernel(uint32_t n_seq, const kgx_call *__restrict__ calls,
                                                        const uint64_t *__restrict__ start,
                                                        const uint32_t *__restrict__ count, kgx_call *__restrict__ ws,
                                                        kgx_best_call *__restrict__ out)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_seq)
        out[s] = best_call_decide(calls + start[s], count[s], ws + start[s]);
}

hipError_t launch_best_calls(uint32_t n_seq, const kgx_call *calls, const uint64_t *start, const uint32_t *count,
                             kgx_call *ws, kgx_best_call *out, hipStream_t stream)
{
    if (n_seq == 0)
        return hipSuccess;
    hipLaunchKernelGGL(best_call_kernel, dim3((n_seq + 255) / 256), dim3(256), 0, stream, n_seq, calls, start,
                       count, ws, out);
    return hipGetLastError();
}

/* ------------------------------------------------------------------------ */
/* OTU tallies: KmerOtuStats (kguts.h:185-219), one lane per sequence         */
/* ------------------------------------------------------------------------ */

/* otu_map[oI]++ over the hits the scorer flagged KGX_HIT_OTU (the hits
 * process_set_of_hits tallies, kguts.cc:760-768), then finalize(): the map's
 * pairs in key order, std::sort by count, larger first (kguts.h:214-218).
 * Scratch: ws / otus of sequence s start at window_base[s] (a sequence has
 * no more flagged hits than windows). */
constexpr int64_t OTU_LDS = 24; /* flagged hits per lane sorted in LDS (24 x 256 x 4 B = 24 KiB) */

template <bool PK>
__global__ __launch_bounds__(256) void otu_kernel(uint32_t n_seq, const uint64_t *__restrict__ wbase,
                                                  const uint64_t *__restrict__ hit_mask, uint32_t tile_windows,
                                                  const uint4 *__restrict__ hot, const uint4 *__restrict__ cold,
                                                  int32_t *__restrict__ ws, kgx_otu *__restrict__ otus,
                                                  uint32_t *__restrict__ otu_count)
{
    typedef HitFields<PK> HF;
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seq)
        return;
    const uint64_t gw0 = wbase[s], gw1 = wbase[s + 1];
    int32_t *v = ws + gw0;
    int64_t n = 0;
    int32_t vmin = INT32_MAX, vmax = INT32_MIN;
    /* the lane's first OTU_LDS values also in LDS: sorting them there avoids
     * a chain of dependent global loads and stores per compare */
    __shared__ int32_t lv[OTU_LDS][256];
    int32_t *mine = &lv[0][threadIdx.x];
    for_each_run(hit_mask, tile_windows, gw0, gw1, [&](uint64_t at0, uint32_t c, uint32_t, uint64_t, uint32_t) {
        for (uint32_t k = 0; k < c; k++) {
            const uint4 h = hot[at0 + k];
            if (HF::flags(h) & KGX_HIT_OTU) {
                const int32_t x = (int32_t)HF::otu(h, PK ? h : cold[at0 + k]);
                if (n < OTU_LDS)
                    mine[256 * n] = x;
                v[n++] = x;
                vmin = min(vmin, x);
                vmax = max(vmax, x);
            }
        }
    });
    int64_t m;
    kgx_otu *o = otus + gw0;
    if (n == 0) {
        m = 0;
    } else if (vmin == vmax) { /* one OTU: otu_map holds one pair, nothing to sort */
        o[0] = kgx_otu{vmin, (int32_t)n};
        m = 1;
    } else if (n <= OTU_LDS) {
        /* the map's keys in order: any sort of plain ints gives the same
         * array (equal values are indistinguishable); insertion sort in LDS */
        for (int64_t i = 1; i < n; i++) {
            const int32_t x = mine[256 * i];
            int64_t j = i - 1;
            while (j >= 0 && mine[256 * j] > x) {
                mine[256 * (j + 1)] = mine[256 * j];
                j--;
            }
            mine[256 * (j + 1)] = x;
        }
        m = 0;
        for (int64_t i = 0; i < n;) {
            int64_t j = i + 1;
            while (j < n && mine[256 * j] == mine[256 * i])
                j++;
            o[m++] = kgx_otu{mine[256 * i], (int32_t)(j - i)};
            i = j;
        }
        /* finalize()'s std::sort of the pairs, replayed (tie order matters) */
        lstd_sort(o, m, [](const kgx_otu &lhs, const kgx_otu &rhs) { return rhs.count < lhs.count; });
    } else {
        m = otu_finalize(v, n, o);
    }
    otu_count[s] = (uint32_t)m;
}

hipError_t launch_otus(uint32_t n_seq, const uint64_t *wbase, const uint64_t *hit_mask, uint32_t tile_windows,
                       const uint4 *hot, const uint4 *cold, int32_t *ws, kgx_otu *otus, uint32_t *otu_count,
                       uint32_t hit_format, hipStream_t stream)
{
    if (n_seq == 0)
        return hipSuccess;
    if (hit_format == HIT_PACKED16)
        hipLaunchKernelGGL(otu_kernel<true>, dim3((n_seq + 255) / 256), dim3(256), 0, stream, n_seq, wbase, hit_mask,
                           tile_windows, hot, cold, ws, otus, otu_count);
    else
        hipLaunchKernelGGL(otu_kernel<false>, dim3((n_seq + 255) / 256), dim3(256), 0, stream, n_seq, wbase,
                           hit_mask, tile_windows, hot, cold, ws, otus, otu_count);
    return hipGetLastError();
}

}  // namespace kgx
