/*
 * kgx_probe.hip -- the probe kernels of the lookup path and their launchers.
 *
 *   probe  : 8-mer encode + linear-probe lookup in the HBM-resident image;
 *            one wave per tile of J*64 consecutive windows of the batch
 *            (across sequence boundaries); J probe chains in flight per lane;
 *            hits compacted per tile in window order with wave ballots
 *
 * In the file's order: the two encodes of a tile (residues, DNA; the key of a
 * window is window_key, kgx_device.h) and the ordered compaction; probe_kernel,
 * one lane per chain; probe_line_kernel, one quad or octet per chain and a
 * table line per load, with the pieces of its aligned body before it -- the
 * hand-over, the test of one line and the chain rules, each defined once and
 * used by both of that body's forms; the launchers, which pick the kernel
 * instance for a batch.
 *
 * Reference behaviour restated (kguts.cc line numbers): residue map 273-339,
 * window set / rolling code 682-732 and 783-871, probe 585-602.
 */
#include <algorithm>
#include <type_traits>

#include "kgx_device.h"

namespace kgx {

/* 12 residue bytes at offset `abo` (a multiple of 4) of the 4-aligned base
 * residues - bm; bytes outside the batch [bm, bm + n) read as 0 (code 20).
 * Offsets and pointer arithmetic, not integer addresses, so the loads stay
 * global loads (a flat load also counts against the LDS wait counter). */
__device__ __forceinline__ uint3 load_residues(const uint8_t *residues, uint64_t bm, uint64_t n, uint64_t abo)
{
    uint32_t d[3] = {0, 0, 0};
    for (int b = 0; b < 12; b++)
        if (abo + b >= bm && abo + b < bm + n)
            d[b >> 2] |= (uint32_t)residues[abo + b - bm] << (8 * (b & 3));
    return make_uint3(d[0], d[1], d[2]);
}

/*
 * One wave = one tile of J*64 windows [g0, g0 + J*64) of the batch.  Lane l
 * owns windows g0 + 64 j + l, so slice j is 64 consecutive windows and its
 * ballot is in window order (= (sequence, position) order).  Every lane
 * finds its window's sequence by walking forward from the tile's first
 * sequence, reads the 8 residues straight from the batch (one 16-byte load),
 * maps them to codes through a 256-byte LDS table, and issues all J first
 * probes before resolving any.
 *   MODE_BUCKET: each probe round loads key and payload of its 24-B bucket;
 *   MODE_KEY_FIRST: rounds load keys only; the matching bucket's payload is
 *     loaded in the round that finds it (mostly the key's sector, in L2);
 *   MODE_PACKED: PACKED16 images -- one aligned 16-B load per bucket gives
 *     key and payload (never straddles a sector; 4 buckets per sector);
 *   MODE_PACKED_KEY_FIRST: the record's low word (key, fI, otu bits) per
 *     bucket, its high word only for the match (same sector).
 */
constexpr int MODE_BUCKET = 0, MODE_KEY_FIRST = 1, MODE_PACKED = 2, MODE_PACKED_KEY_FIRST = 3;

/* a table record; NT = non-temporal (streaming) load, so the random
 * table traffic need not displace a cache-resident presence filter */
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ uint4 load_record(const uint4 *p)
{
    if (NT) {
        const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    return *p;
}

/* the J windows g0 + 64 j + lane of a tile: their keys (big-endian base-20
 * codes, encoded_kmer kguts.cc:438-455), whether they are valid (inside the
 * batch, no code-20 residue: advance_past_ambig), and their (seq, pos) */
template <int J>
__device__ __forceinline__ void encode_tile(const uint8_t *__restrict__ residues, uint64_t n_residues,
                                            const uint64_t *__restrict__ seq_off,
                                            const uint64_t *__restrict__ wbase, uint32_t s,
                                            uint64_t W, uint64_t g0, uint32_t lane,
                                            const uint8_t *code_tab, uint64_t *key, bool *ok,
                                            uint32_t *pos, uint32_t *sq, uint32_t *a7 = nullptr,
                                            uint32_t *b7 = nullptr)
{
    /* byte offsets from residues - bm, which is 4-aligned */
    const uint64_t bm = reinterpret_cast<uintptr_t>(residues) & 3;
    uint64_t wb_lo = wbase[s], wb_hi = wbase[s + 1], soff = seq_off[s];
    uint64_t ab[J];
    uint32_t sh[J];
    uint4 v[J];
    bool fast[J];
    /* pass 1: each window's sequence, and one 16-byte load of its residues,
     * issued for all J windows before any is used (a window whose 16 bytes
     * would leave the batch is read bytewise in pass 2).  Loads under a
     * divergent branch stay in flight past the join only when the loaded
     * variable holds nothing older to merge with -- here and in the probes,
     * such variables are written once per round. */
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint64_t gw = g0 + 64 * j + lane;
        const bool act = gw < W;
        while (act && gw >= wb_hi) { /* next sequence (skips window-less ones) */
            s++;
            wb_lo = wb_hi;
            wb_hi = wbase[s + 1];
            soff = seq_off[s];
        }
        pos[j] = (uint32_t)(gw - wb_lo);
        sq[j] = s;
        const uint64_t a = bm + soff + (gw - wb_lo);
        ab[j] = a & ~3ull;
        sh[j] = (uint32_t)(a - ab[j]);
        ok[j] = act;
        fast[j] = ab[j] >= bm && ab[j] + 16 <= bm + n_residues;
        if (fast[j])
            v[j] = *reinterpret_cast<const uint4 *>(residues + (ab[j] - bm));
    }
    /* pass 2: codes and keys */
#pragma unroll
    for (int j = 0; j < J; j++) {
        uint3 d = make_uint3(v[j].x, v[j].y, v[j].z);
        if (!fast[j])
            d = load_residues(residues, bm, n_residues, ab[j]);
        const uint32_t lo = __builtin_amdgcn_alignbyte(d.y, d.x, sh[j]);
        const uint32_t hi = __builtin_amdgcn_alignbyte(d.z, d.y, sh[j]);
        const uint32_t c0 = code_tab[lo & 0xFF], c1 = code_tab[(lo >> 8) & 0xFF],
                       c2 = code_tab[(lo >> 16) & 0xFF], c3 = code_tab[lo >> 24];
        const uint32_t c4 = code_tab[hi & 0xFF], c5 = code_tab[(hi >> 8) & 0xFF],
                       c6 = code_tab[(hi >> 16) & 0xFF], c7 = code_tab[hi >> 24];
        window_key(WindowCodes{{c0, c1, c2, c3, c4, c5, c6, c7}}, key[j], ok[j]);
        if (a7) { /* the key's two 7-mers, for the home (kgx_line_home.h) */
            const uint32_t cc[8] = {c0, c1, c2, c3, c4, c5, c6, c7};
            seven_mers(cc, a7[j], b7[j]);
        }
    }
}

/*
 * The same J windows when the batch is the fq path's fragments left as DNA
 * (kgx_fq_run_device): fragment s is a run of codons of one frame of a read,
 * described by anchor[s] = (byte index of its first codon's first base) << 1
 * | reverse.  Forward, codon i is bases A+3i..A+3i+2; on the reverse strand it
 * is the complement of bases A-3i, A-3i-1, A-3i-2 (frame -k read backwards,
 * dna_seq.cc:9-47).  A window's 8 codons are the 24 bytes from A+3p (forward)
 * or ending at A-3p (reverse), loaded as two 16-B reads; each base becomes
 * its class through cls_tab (A0 C1 G2 T/U3, anything else 0x40, so a codon
 * with a non-base indexes past 63) and each codon its residue code through
 * cod_tab.  A reverse window's 24 bytes are reversed first (byte swaps), so
 * codon i is bytes 3i..3i+2 either way and its index is complemented by xor
 * 63.  The keys equal encode_tile's over the translated residues
 * (kgx_fq_fragments with residues).
 */
template <int J>
__device__ __forceinline__ void encode_tile_dna(const uint8_t *__restrict__ bases, uint64_t n_bases,
                                                const uint64_t *__restrict__ anchor,
                                                const uint64_t *__restrict__ wbase, uint32_t s, uint64_t W,
                                                uint64_t g0, uint32_t lane, const uint8_t *cls_tab,
                                                const uint8_t *cod_tab, uint64_t *key, bool *ok, uint32_t *pos,
                                                uint32_t *sq, uint32_t *a7 = nullptr, uint32_t *b7 = nullptr)
{
    const uint64_t bm = reinterpret_cast<uintptr_t>(bases) & 3;
    uint64_t wb_lo = wbase[s], wb_hi = wbase[s + 1], an = anchor[s];
    uint64_t ab[J], lo[J];
    uint32_t sh[J];
    uint4 v0[J], v1[J];
    bool fast[J], rev[J];
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint64_t gw = g0 + 64 * j + lane;
        const bool act = gw < W;
        while (act && gw >= wb_hi) {
            s++;
            wb_lo = wb_hi;
            wb_hi = wbase[s + 1];
            an = anchor[s];
        }
        const uint64_t p = gw - wb_lo;
        pos[j] = (uint32_t)p;
        sq[j] = s;
        rev[j] = an & 1u;
        const uint64_t A = an >> 1;
        lo[j] = act ? (rev[j] ? A - 3 * p - 23 : A + 3 * p) : 0; /* the window's first byte */
        const uint64_t a = bm + lo[j];
        ab[j] = a & ~3ull;
        sh[j] = (uint32_t)(a - ab[j]);
        ok[j] = act;
        fast[j] = act && ab[j] >= bm && ab[j] + 32 <= bm + n_bases;
        if (fast[j]) {
            const uint4 *q = reinterpret_cast<const uint4 *>(bases + (ab[j] - bm));
            v0[j] = q[0];
            v1[j] = q[1];
        }
    }
#pragma unroll
    for (int j = 0; j < J; j++) {
        uint32_t d[6];
        if (fast[j]) {
            const uint32_t w[7] = {v0[j].x, v0[j].y, v0[j].z, v0[j].w, v1[j].x, v1[j].y, v1[j].z};
#pragma unroll
            for (int k = 0; k < 6; k++)
                d[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh[j]);
        } else { /* near the buffer's end (or inactive): byte by byte */
#pragma unroll
            for (int k = 0; k < 6; k++)
                d[k] = 0;
            if (ok[j])
                for (int i = 0; i < 24; i++)
                    d[i >> 2] |= (uint32_t)bases[lo[j] + i] << (8 * (i & 3));
        }
        /* reverse strand: the span's bytes reversed, so that codon i is bytes
         * 3i..3i+2 either way (its index then complemented: xor 63) */
        uint32_t rd[6];
#pragma unroll
        for (int k = 0; k < 6; k++)
            rd[k] = __builtin_bswap32(d[5 - k]);
#pragma unroll
        for (int k = 0; k < 6; k++)
            d[k] = rev[j] ? rd[k] : d[k];
        const uint32_t flip = rev[j] ? 63u : 0u;
        uint32_t c[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int b0 = 3 * i, b1 = 3 * i + 1, b2 = 3 * i + 2;
            const uint32_t e1 = cls_tab[(d[b0 >> 2] >> (8 * (b0 & 3))) & 0xFFu];
            const uint32_t e2 = cls_tab[(d[b1 >> 2] >> (8 * (b1 & 3))) & 0xFFu];
            const uint32_t e3 = cls_tab[(d[b2 >> 2] >> (8 * (b2 & 3))) & 0xFFu];
            const uint32_t e = ((e1 << 4) | (e2 << 2) | e3) ^ flip; /* >= 64: a non-base */
            c[i] = cod_tab[min(e, 64u)]; /* unconditional read: entry 64 = 20 */
        }
        window_key(WindowCodes{{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]}}, key[j], ok[j]);
        if (a7)
            seven_mers(c, a7[j], b7[j]);
    }
}

/* ordered compaction of a tile's hits; one mask word per slice.  PACKED:
 * pv = the matching PACKED16 record, stored as is (HIT_PACKED16); else pv =
 * the 16 B after the key of the matching AOS24 bucket, stored as the two
 * planes (HIT_PLANES) */
template <int J, bool PACKED>
__device__ __forceinline__ void store_tile_hits(const bool *hit, const uint64_t *kv, const uint4 *pv,
                                                const uint32_t *pos, const uint32_t *sq, uint64_t g0,
                                                uint64_t W, uint32_t lane, uint4 *__restrict__ hot,
                                                uint4 *__restrict__ cold,
                                                uint64_t *__restrict__ hit_mask, bool nt = false)
{
    uint32_t count = 0;
#pragma unroll
    for (int j = 0; j < J; j++) {
        const uint64_t m = __ballot(hit[j]);
        if (hit[j]) {
            const uint64_t at = g0 + count + lanes_below(m);
            /* HIT_PACKED16: the table record itself, less its share of an
             * index line's overflow marks (kgx_line_home.h): those bits are
             * the scorer's flags in a hit and leave the probe clear */
            const uint32_t w = pv[j].w & ~MARK_BITS_W;
            if (PACKED && nt) {
                typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
                const u32x4_t v = {pv[j].x, pv[j].y, pv[j].z, w};
                __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t *>(hot + at));
            } else if (PACKED) {
                hot[at] = make_uint4(pv[j].x, pv[j].y, pv[j].z, w);
            } else {
                hot[at] = make_uint4(pv[j].y & 0xFFFFu, pv[j].z, pv[j].w, pos[j]);
                cold[at] = make_uint4((uint32_t)kv[j], (uint32_t)(kv[j] >> 32), pv[j].x, sq[j]);
            }
        }
        if (lane == 0 && g0 + 64 * j < W) {
            if (nt)
                __builtin_nontemporal_store(m, hit_mask + (g0 >> 6) + j);
            else
                hit_mask[(g0 >> 6) + j] = m;
        }
        count += (uint32_t)__popcll(m);
    }
}

template <int J, int MODE, bool FILTER, bool NT = FILTER>
__global__ __launch_bounds__(256) void probe_kernel(
    const uint8_t *__restrict__ residues, uint64_t n_residues, const uint64_t *__restrict__ seq_off,
    const uint64_t *__restrict__ wbase, const uint32_t *__restrict__ tile_seq, uint32_t n_seq,
    const void *__restrict__ table_v, uint64_t num_sigs, uint64_t magic, uint32_t home,
    const uint64_t *__restrict__ filter, uint32_t filter_log2,
    uint4 *__restrict__ hot, uint4 *__restrict__ cold, uint64_t *__restrict__ hit_mask)
{
    constexpr bool KEY_FIRST = MODE == MODE_KEY_FIRST;
    constexpr bool PACKED = MODE == MODE_PACKED || MODE == MODE_PACKED_KEY_FIRST;
    const uint64_t *__restrict__ packed_w = static_cast<const uint64_t *>(table_v);
    const kgx_sig_kmer *__restrict__ table = static_cast<const kgx_sig_kmer *>(table_v);
    const uint4 *__restrict__ packed = static_cast<const uint4 *>(table_v);
    constexpr uint32_t T = 64 * J;
    __shared__ uint8_t code_tab[256];
    code_tab[threadIdx.x] = (uint8_t)residue_code(threadIdx.x);
    __syncthreads();

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = lane_id();
    const uint64_t W = wbase[n_seq];
    const uint64_t tile = (uint64_t)blockIdx.x * PROBE_WAVES + wave;
    const uint64_t g0 = tile * T;
    if (g0 >= W)
        return;

    uint64_t key[J], slot[J], fw[J];
    uint32_t pos[J], sq[J];
    bool pend[J], hit[J];
    encode_tile<J>(residues, n_residues, seq_off, wbase, tile_seq[tile], W, g0, lane, code_tab, key,
                   pend, pos, sq);
#pragma unroll
    for (int j = 0; j < J; j++) {
        hit[j] = false;
        fw[j] = 0;
        if (FILTER && pend[j]) /* presence filter word (MALL-resident): issue now, test below */
            fw[j] = filter[filter_word(filter_hash(key[j]), filter_log2)];
    }
#pragma unroll
    for (int j = 0; j < J; j++) {
        if (FILTER && pend[j]) {
            const uint64_t m = filter_bits(filter_hash(key[j]));
            pend[j] = (fw[j] & m) == m; /* else stored nowhere: a miss */
        }
        slot[j] = pend[j] ? home_bucket(key[j], num_sigs, magic, home) : 0; /* home: kgx_line_home.h */
    }

    uint4 rec[J]; /* the matching bucket's payload */
#pragma unroll
    for (int j = 0; j < J; j++)
        rec[j] = make_uint4(0, 0, 0, 0);

    /* linear probe rounds (lookup_hash_entry, kguts.cc:585-602); bounded by
     * num_sigs buckets where the reference would spin forever */
    for (uint64_t round = 0;; round++) {
        /* bucket slot[j] of every pending window, all J in flight at once */
        uint4 pv[J];
        uint64_t kv[J];
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (pend[j]) {
                if (MODE == MODE_PACKED) {
                    pv[j] = load_record<NT>(packed + slot[j]);
                } else if (MODE == MODE_PACKED_KEY_FIRST) {
                    const uint64_t lo = packed_w[2 * slot[j]];
                    pv[j].x = (uint32_t)lo;
                    pv[j].y = (uint32_t)(lo >> 32);
                } else {
                    const kgx_sig_kmer *e = table + slot[j];
                    kv[j] = e->which_kmer;
                    if (!KEY_FIRST)
                        pv[j] = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(e) + 8);
                }
            }
        }
        bool more = false;
#pragma unroll
        for (int j = 0; j < J; j++) {
            if (PACKED)
                kv[j] = ((uint64_t)pv[j].y << 32 | pv[j].x) & PACK_KEY_MASK;
            /* straight-line selects: a branch here would let the compiler
             * split the record load and re-read its payload half on a match */
            const bool m = pend[j] && kv[j] == key[j];
            const bool stop = kv[j] > MAX_ENCODED || round + 1 >= num_sigs;
            if (!KEY_FIRST && MODE != MODE_PACKED_KEY_FIRST) { /* per component: a select of */
                rec[j].x = m ? pv[j].x : rec[j].x;               /* whole uint4s goes through */
                rec[j].y = m ? pv[j].y : rec[j].y;               /* scratch memory */
                rec[j].z = m ? pv[j].z : rec[j].z;
                rec[j].w = m ? pv[j].w : rec[j].w;
            }
            if ((KEY_FIRST || MODE == MODE_PACKED_KEY_FIRST) && m) {
                if (KEY_FIRST)
                    rec[j] = *reinterpret_cast<const uint4 *>(
                        reinterpret_cast<const char *>(table + slot[j]) + 8);
                if (MODE == MODE_PACKED_KEY_FIRST) {
                    const uint64_t hi = packed_w[2 * slot[j] + 1];
                    rec[j] = make_uint4(pv[j].x, pv[j].y, (uint32_t)hi, (uint32_t)(hi >> 32));
                }
            }
            hit[j] = hit[j] || m;
            pend[j] = pend[j] && !m && !stop;
            slot[j] = pend[j] ? (slot[j] + 1 == num_sigs ? 0 : slot[j] + 1) : slot[j];
            more = more || pend[j];
        }
        if (!__any(more))
            break;
    }

    store_tile_hits<J, PACKED>(hit, key, rec, pos, sq, g0, W, lane, hot, cold, hit_mask);
}

/*
 * Cooperative-line probe of a PACKED16 image.  The encode and the ordered
 * compaction are probe_kernel's; the lookups are done by groups of G lanes
 * that read one aligned G*16-byte line of the table in one instruction (lane
 * c of the group holds bucket line + c).  A wave instruction serves 64 / G
 * windows, and a linear-probe chain costs one line request per line it
 * touches instead of one request per bucket: about 1.07 requests per window
 * instead of P-bar = 1.33 (the chip's ceiling is random line requests, and
 * 64-B lines read this way run at 45 G/s, tools/line_probe.py).
 *
 * Window w of the tile (w = 64 j + l, owned by lane l in slice j) is looked
 * up by group q = l % (64 / G) in instruction i = l / (64 / G) of slice j.  The group
 * examines buckets in probe order: from the home slot to the end of its line,
 * then whole lines, wrapping at num_sigs; the first bucket whose key matches
 * (hit) or exceeds MAX_ENCODED (miss) ends the chain -- lookup_hash_entry,
 * kguts.cc:585-602.  A chain that has covered the whole table without either
 * is a miss (the reference spins forever there; probe_kernel stops after
 * num_sigs buckets -- same answer, since every bucket has been seen).
 * The matching lane writes the record to LDS for the window's owner.
 *
 * Over an aligned index (line_index_aligned, kgx_line_home.h: whole 4-record
 * lines, line-aligned homes, overflow marks, fewer than 2^32 - 2 lines) the
 * chain rules are those of the kernel's generic slice; what the alignment
 * settles is left out: a chain's position is a 32-bit line number, every
 * record of a line belongs to the chain and lies inside the table, and a line
 * searched in vain was searched whole, so its overflow mark for the key
 * decides whether the chain goes on.  Both forms of the aligned body -- rounds
 * per slice (probe_slice_aligned) and deferred (probe_slice_round0, then
 * probe_tile_deferred) -- are made of the pieces that follow, each rule
 * defined once.
 */
constexpr uint32_t LINE_G = 4, LINE_NQ = 64 / LINE_G; /* the index's records per line; windows per instruction */
constexpr uint32_t MARKED = 1u << LINE_G;             /* in a line's word: the line carries the key's mark */
constexpr uint32_t KEY_HI = (uint32_t)(PACK_KEY_MASK >> 32);
static_assert(KEY_HI == 7u && (MARK_BITS_W & KEY_HI) == 0, "key bits 32-34 beside the mark bit");

/* what a window's owner hands its quad beside the key's low word and the home
 * line: key bits 32-34, the open-chain bit, line_mark of the key from bit 4 */
__device__ __forceinline__ uint32_t owner_word(uint64_t key, bool ok)
{
    return (uint32_t)(key >> 32) | (uint32_t)ok << 3 | line_mark(key) << 4;
}
/* what lane c of the quad keeps of an owner's word: the key's high bits and
 * the one bit of its own record's last dword that holds the key's mark (or
 * none) in one word: bits 0-2 and 28-31 do not meet */
__device__ __forceinline__ uint32_t lane_key_word(uint32_t own, uint32_t c)
{
    const uint32_t g = own >> 4;
    return (own & KEY_HI) | (c == mark_record(g) ? 1u << mark_bit_w(g) : 0u);
}
/* The hand-over: lane c of quad q takes the quad's G chains of a slice from
 * their owners, lane NQ i + q for instruction i.  Returns the open chains,
 * bit i for instruction i. */
__device__ __forceinline__ uint32_t quad_hand_over(uint64_t key, uint32_t own, uint32_t home_line, uint32_t q, uint32_t c,
                                                   uint32_t (&klo)[LINE_G], uint32_t (&kw)[LINE_G],
                                                   uint32_t (&ln)[LINE_G])
{
    uint32_t live = 0;
#pragma unroll
    for (int i = 0; i < (int)LINE_G; i++) {
        const int owner = (int)(LINE_NQ * i + q);
        klo[i] = (uint32_t)__shfl((int)(uint32_t)key, owner);
        ln[i] = (uint32_t)__shfl((int)home_line, owner);
        const uint32_t o = (uint32_t)__shfl((int)own, owner);
        live |= (o >> 3 & 1u) << i;
        kw[i] = lane_key_word(o, c);
    }
    return live;
}

/* The test of one line, d = this lane's record of it (cbit = 1 << c): the
 * line's word, ORed over the quad by two DPP moves (a quad is the lanes of one
 * line, and every lane of the wave is active here) -- bit c, record c holds
 * the key or is empty; MARKED, the line carries the key's mark; 0 for a closed
 * chain -- and `diff`, 0 where this lane's record holds the key.
 * The record's key is tested in its two words, and for equality through xor:
 * after `d.x == klo` the compiler hands over klo in d.x's place, and after a
 * 64-bit compare it builds a register pair in the loaded one's; either way the
 * record is put together again by copies that wait for the load at the branch
 * join.  `> MAX_ENCODED` is two 32-bit tests for the same reason. */
__device__ __forceinline__ uint32_t quad_line_word(const uint4 &d, uint32_t klo, uint32_t kw, bool open,
                                                   uint32_t cbit, uint32_t &diff)
{
    constexpr uint32_t MAX_HI = (uint32_t)(MAX_ENCODED >> 32), MAX_LO = (uint32_t)MAX_ENCODED;
    const uint32_t kh = d.y & KEY_HI;
    diff = (d.x ^ klo) | ((d.y ^ kw) & KEY_HI);
    const bool ends = diff == 0 || kh > MAX_HI || (kh == MAX_HI && d.x > MAX_LO);
    uint32_t w = (ends ? cbit : 0u) | ((d.w & kw) >= 1u << 28 ? MARKED : 0u);
    w = open ? w : 0u;
    w |= (uint32_t)xor_lane((int32_t)w, 1);
    w |= (uint32_t)xor_lane((int32_t)w, 2);
    return w;
}
/* the line's first match or empty bucket ends the chain; a match there is the
 * hit: this lane's record (diff 0), none of the line's word set before it
 * (cbit = 1 << c, this lane's record; upto = (2 << c) - 1, it and those before) */
__device__ __forceinline__ bool lane_hits(uint32_t diff, uint32_t w, uint32_t cbit, uint32_t upto)
{
    return diff == 0 && (w & upto) == cbit;
}
/* on: nothing found, and the key's mark set (a full line whose mark for the
 * key is clear was never passed by it) */
__device__ __forceinline__ bool chain_goes_on(uint32_t w) { return (w & (2u * MARKED - 1)) == MARKED; }
__device__ __forceinline__ uint32_t next_line(uint32_t ln, uint32_t n_lines) { return ln + 1 == n_lines ? 0 : ln + 1; }

/* a 64-window slice to its end; `rec` and `hitf` are its 64 hand-over slots in LDS */
__device__ __forceinline__ void probe_slice_aligned(const uint4 *__restrict__ packed, uint32_t n_lines, uint64_t key,
                                                    bool ok, uint32_t home_line, uint32_t q, uint32_t c, uint4 *rec,
                                                    uint8_t *hitf)
{
    constexpr uint32_t G = LINE_G, NQ = LINE_NQ;
    uint32_t klo[G], kw[G], ln[G];
    uint32_t live = quad_hand_over(key, owner_word(key, ok), home_line, q, c, klo, kw, ln); /* bit i: chain i is open */
    const uint32_t cbit = 1u << c, upto = (2u << c) - 1u;
    const uint32_t max_lines = n_lines + 2; /* lines a chain may visit before it has covered the table */
    for (uint32_t round = 0;; round++) {
        /* only open chains load; d is fresh each round (no merge with an
         * older value at the branch join, so no wait for the load there) */
        uint4 d[G];
#pragma unroll
        for (int i = 0; i < (int)G; i++)
            if (live >> i & 1u)
                d[i] = packed[(uint64_t)ln[i] * G + c];
        uint32_t hitm = 0; /* bit i: this lane's record is instruction i's hit */
#pragma unroll
        for (int i = 0; i < (int)G; i++) {
            uint32_t diff;
            const uint32_t w = quad_line_word(d[i], klo[i], kw[i], live >> i & 1u, cbit, diff);
            hitm |= lane_hits(diff, w, cbit, upto) ? 1u << i : 0u;
            live = chain_goes_on(w) ? live : live & ~(1u << i);
            ln[i] = next_line(ln[i], n_lines);
        }
        /* the hits are handed to the windows' owners after all four tests:
         * no branch stands between the tests, so their instructions mix */
#pragma unroll
        for (int i = 0; i < (int)G; i++)
            if (hitm >> i & 1u) {
                rec[NQ * i + q] = d[i];
                hitf[NQ * i + q] = 1;
            }
        if (round + 1 >= max_lines) /* the table covered */
            live = 0;
        if (!__any(live != 0))
            break;
    }
}

/*
 * The deferred form of the aligned slice (DEFER, the default; environment
 * switch KGX_PROBE_DEFER): a tile's chains that leave their first line are not
 * walked slice by slice, a few lanes at a time at the whole round's cost, but
 * once for the tile, packed 16 to a load instruction.
 *
 * Round 0 of a 64-window slice, straight-line: the hand-over and one round
 * without the loop -- the round of probe_slice_aligned, written out again
 * because a function shared by the two changes what the compiler makes of
 * both.  Returns the quad's open chains, bit i for instruction i (the same in
 * the quad's four lanes); their next line is the one after the home.
 */
__device__ __forceinline__ uint32_t probe_slice_round0(const uint4 *__restrict__ packed, uint64_t key, uint32_t own,
                                                       uint32_t home_line, uint32_t q, uint32_t c, uint4 *rec,
                                                       uint8_t *hitf)
{
    constexpr uint32_t G = LINE_G, NQ = LINE_NQ;
    uint32_t klo[G], kw[G], ln[G];
    uint32_t live = quad_hand_over(key, own, home_line, q, c, klo, kw, ln);
    const uint32_t cbit = 1u << c, upto = (2u << c) - 1u;
    uint4 d[G];
#pragma unroll
    for (int i = 0; i < (int)G; i++)
        if (live >> i & 1u)
            d[i] = packed[(uint64_t)ln[i] * G + c];
    uint32_t hitm = 0;
#pragma unroll
    for (int i = 0; i < (int)G; i++) {
        uint32_t diff;
        const uint32_t w = quad_line_word(d[i], klo[i], kw[i], live >> i & 1u, cbit, diff);
        hitm |= lane_hits(diff, w, cbit, upto) ? 1u << i : 0u;
        live = chain_goes_on(w) ? live : live & ~(1u << i);
    }
#pragma unroll
    for (int i = 0; i < (int)G; i++)
        if (hitm >> i & 1u) {
            rec[NQ * i + q] = d[i];
            hitf[NQ * i + q] = 1;
        }
    return live;
}

/* The tile's n_open chains left open by round 0, in window order in `list`
 * (window slots of the tile); chain w's entry lies in rec[w], which is free
 * until the chain hits: key low word, owner_word (its key bits 32-34 and
 * line_mark are used), next line.  Quad q walks entry
 * 16 p + q of pass p, all 16 in one load instruction per round, by
 * probe_slice_aligned's rules; a chain has visited one line already, so the
 * rounds count from 1 towards the n_lines + 2 that cover the table. */
__device__ __forceinline__ void probe_tile_deferred(const uint4 *__restrict__ packed, uint32_t n_lines,
                                                    uint32_t n_open, const uint8_t *list, uint32_t q, uint32_t c,
                                                    uint4 *rec, uint8_t *hitf)
{
    constexpr uint32_t G = LINE_G, NQ = LINE_NQ;
    const uint32_t cbit = 1u << c, upto = (2u << c) - 1u;
    const uint32_t max_lines = n_lines + 2;
    for (uint32_t p = 0; p < n_open; p += NQ) {
        bool live = p + q < n_open;
        uint32_t w = 0;
        uint4 e = make_uint4(0, 0, 0, 0);
        if (live) {
            w = list[p + q];
            e = rec[w];
        }
        const uint32_t klo = e.x, kw = lane_key_word(e.y, c);
        uint32_t ln = e.z;
        for (uint32_t round = 1;; round++) {
            uint4 d; /* fresh each round, as in probe_slice_aligned */
            if (live)
                d = packed[(uint64_t)ln * G + c];
            uint32_t diff;
            const uint32_t lw = quad_line_word(d, klo, kw, live, cbit, diff);
            if (lane_hits(diff, lw, cbit, upto)) {
                rec[w] = d;
                hitf[w] = 1;
            }
            const bool on = chain_goes_on(lw);
            live = live && on && round + 1 < max_lines;
            ln = next_line(ln, n_lines);
            if (!__any(live))
                break;
        }
    }
}

/* The static LDS of a line probe workgroup at the default J = 2, which is what
 * launch_probe takes off a probe_lds_kb reservation: a 128-window tile's
 * 8960 B (the code table's 256, 4 waves x 128 windows of 16-B hand-over
 * records and of hit flags) counted as 9 KB, and with the deferred form's list
 * of open chains, 4 x 128 B more. */
constexpr uint32_t PROBE_LINE_LDS = 9216, PROBE_LINE_LDS_DEFER = PROBE_LINE_LDS + 512;

template <int J, int G, bool DNA, bool MARKS, bool TWINS, bool DEFER>
__global__ __launch_bounds__(256) void probe_line_kernel(
    const uint8_t *__restrict__ residues, uint64_t n_residues, const uint64_t *__restrict__ seq_off,
    const uint64_t *__restrict__ wbase, const uint32_t *__restrict__ tile_seq, uint32_t n_seq,
    const uint4 *__restrict__ packed, uint64_t num_sigs, uint64_t magic, uint32_t home, uint4 *__restrict__ hot,
    uint4 *__restrict__ cold, uint64_t *__restrict__ hit_mask, uint32_t nt)
{
    constexpr uint32_t T = 64 * J;
    constexpr uint32_t NQ = 64 / G; /* windows per instruction */
    __shared__ uint8_t code_tab[256]; /* residue -> code; DNA: base -> class */
    __shared__ uint8_t cod_tab[DNA ? 68 : 1];
    __shared__ uint4 lds_rec[PROBE_WAVES][T];
    __shared__ uint8_t lds_hit[PROBE_WAVES][T];
    __shared__ uint8_t lds_open[PROBE_WAVES][DEFER ? T : 1]; /* DEFER: the tile's open chains (window slots) */
    static_assert(T <= 256, "a window slot is a byte of lds_open");
    static_assert(J != 2 || sizeof(code_tab) + sizeof(cod_tab) + sizeof(lds_rec) + sizeof(lds_hit) + sizeof(lds_open) <=
                                (DEFER ? PROBE_LINE_LDS_DEFER : PROBE_LINE_LDS),
                  "the launcher's count of this LDS");
    if (DNA) {
        const uint32_t b = threadIdx.x | 0x20u; /* ACGTU either case (trans_table.h:45-68) */
        const bool base = b == 'a' || b == 'c' || b == 'g' || b == 't' || b == 'u';
        code_tab[threadIdx.x] = base ? (uint8_t)(((b >> 1) ^ (b >> 2)) & 3u) : (uint8_t)0x40;
        if (threadIdx.x < 65)
            cod_tab[threadIdx.x] = threadIdx.x < 64 ? (uint8_t)residue_code((uint8_t)code11_aa(threadIdx.x)) : 20;
    } else {
        code_tab[threadIdx.x] = (uint8_t)residue_code(threadIdx.x);
    }
    __syncthreads();

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = lane_id();
    const uint64_t W = wbase[n_seq];
    /* one tile per wave, or (a grid smaller than the tiles, option
     * probe_persist) the wave strides over tiles: every wave leaves once its
     * next tile lies past the batch's last window */
    for (uint64_t tile = (uint64_t)blockIdx.x * PROBE_WAVES + wave; tile * T < W;
         tile += (uint64_t)gridDim.x * PROBE_WAVES) {
        const uint64_t g0 = tile * T;

        uint64_t key[J];
        uint32_t pos[J], sq[J];
        bool ok[J];
        const uint32_t q = lane / G, c = lane % G;
        /* MARKS: the table is an aligned index (the launcher: line_index_aligned,
         * G = 4).  Its homes come from the 7-mers the encode holds and its slices
         * run probe_slice_aligned; without, the kernel is the generic one below
         * and holds none of the aligned body's instructions or registers */
        /* TWINS: the index holds every key under the homes of both its 7-mers
         * (kgx_line_home.h), and a window starts at pair_home of its index in the
         * batch: g0, 64 j and the 16 windows of an instruction are all even, so
         * windows g (even) and g + 1 are neighbouring quads of one instruction
         * and, in one sequence, ask for one line.  Under pairs (sp = 1) the
         * shared 7-mer owns a 128-byte block and the two windows start on its
         * halves, lines 2h and 2h + 1: eight lanes on one aligned block */
        static_assert(!MARKS || G == 4, "the index's lines are 4 records");
        static_assert(!TWINS || MARKS, "twin records come with marks only");
        if constexpr (MARKS) {
            uint32_t a7[J], b7[J];
            if (DNA)
                encode_tile_dna<J>(residues, n_residues, seq_off, wbase, tile_seq[tile], W, g0, lane, code_tab,
                                   cod_tab, key, ok, pos, sq, a7, b7);
            else
                encode_tile<J>(residues, n_residues, seq_off, wbase, tile_seq[tile], W, g0, lane, code_tab, key, ok,
                               pos, sq, a7, b7);
            const uint32_t n_lines = (uint32_t)(num_sigs / G);
            const uint32_t sp = home_pairs_of(home) ? 1u : 0u, n_homes = n_lines >> sp; /* magic is n_homes' */
            uint32_t home_line[J];
#pragma unroll
            for (int j = 0; j < J; j++) {
                if (TWINS) /* g's parity is the lane's */
                    home_line[j] = ok[j] ? (uint32_t)pair_home(a7[j], b7[j], lane, n_homes, magic) << sp | (lane & sp) : 0;
                else
                    home_line[j] = ok[j] ? (uint32_t)line_home_7mers(a7[j], b7[j], n_lines, magic, home_mode_of(home)) : 0;
                lds_hit[wave][64 * j + lane] = 0;
            }
            if constexpr (DEFER) {
                /* each slice's first round, then the tile's open chains together.
                 * A window's owner learns from its quad (lanes 4 (l % 16) on,
                 * instruction l / 16) whether the chain is open and files it: the
                 * ballot is in window order, so under TWINS an even window and
                 * its successor are neighbouring quads of a deferred instruction
                 * too (unless a pass boundary parts them) and ask for one line */
                uint32_t n_open = 0; /* per tile: a wave may walk many */
#pragma unroll
                for (int j = 0; j < J; j++) {
                    const uint32_t own = owner_word(key[j], ok[j]);
                    const uint32_t live = probe_slice_round0(packed, key[j], own, home_line[j], q, c,
                                                             &lds_rec[wave][64 * j], &lds_hit[wave][64 * j]);
                    const uint32_t of_quad = (uint32_t)__shfl((int)live, (int)(G * (lane % NQ)));
                    const bool open = of_quad >> (lane / NQ) & 1u;
                    const uint64_t m = __ballot(open);
                    if (open) {
                        lds_rec[wave][64 * j + lane] = make_uint4((uint32_t)key[j], own, next_line(home_line[j], n_lines), 0);
                        lds_open[wave][n_open + lanes_below(m)] = (uint8_t)(64 * j + lane);
                    }
                    n_open += (uint32_t)__popcll(m);
                }
                wave_lds_sync();
                probe_tile_deferred(packed, n_lines, n_open, lds_open[wave], q, c, lds_rec[wave], lds_hit[wave]);
            } else {
                /* one 64-window slice at a time, as below */
#pragma unroll
                for (int j = 0; j < J; j++)
                    probe_slice_aligned(packed, n_lines, key[j], ok[j], home_line[j], q, c, &lds_rec[wave][64 * j],
                                        &lds_hit[wave][64 * j]);
            }
        } else {
            if (DNA)
                encode_tile_dna<J>(residues, n_residues, seq_off, wbase, tile_seq[tile], W, g0, lane, code_tab, cod_tab,
                                   key, ok, pos, sq);
            else
                encode_tile<J>(residues, n_residues, seq_off, wbase, tile_seq[tile], W, g0, lane, code_tab, key, ok,
                               pos, sq);
            uint64_t first[J]; /* the chain's first bucket */
#pragma unroll
            for (int j = 0; j < J; j++) {
                first[j] = ok[j] ? home_bucket(key[j], num_sigs, magic, home) : 0; /* line starts with the index */
                lds_hit[wave][64 * j + lane] = 0;
            }

            /* lines a chain may visit before it has covered the whole table */
            const uint64_t max_lines = num_sigs / G + 2;
            /* One 64-window slice (G instructions) at a time, each with its own
             * rounds: the wave holds G lines in flight instead of J * G, so a tile of
             * any J needs the registers of J = 1 (8 waves per SIMD at G = 4, where
             * all of a 128-window tile's chains at once left 5).  With the minimizer
             * home nearly every wave runs a second, almost empty round, and it is
             * the other resident waves that cover it. */
#pragma unroll
            for (int j = 0; j < J; j++) {
                uint64_t K[G], cur[G];
                /* bit i: instruction i's chain is still open */
                uint32_t live = 0;
                const uint32_t own = (uint32_t)ok[j];
#pragma unroll
                for (int i = 0; i < G; i++) {
                    const uint32_t owner = NQ * i + q;
                    K[i] = __shfl(key[j], (int)owner);
                    cur[i] = __shfl(first[j], (int)owner);
                    const uint32_t o = (uint32_t)__shfl((int)own, (int)owner);
                    live |= (o & 1u) << i;
                }
                for (uint64_t round = 0;; round++) {
                    /* only open chains load; d is fresh each round (no merge with an
                     * older value at the branch join, so no wait for the load there) */
                    uint4 d[G];
#pragma unroll
                    for (int i = 0; i < G; i++) {
                        const uint64_t line = cur[i] - cur[i] % G;
                        if ((live >> i & 1u) && line + c < num_sigs)
                            d[i] = packed[line + c];
                    }
                    bool more = false;
#pragma unroll
                    for (int i = 0; i < G; i++) {
                        const bool act = live >> i & 1u;
                        const uint64_t line = cur[i] - cur[i] % G;
                        const uint64_t b = line + c;
                        const uint64_t kb = ((uint64_t)d[i].y << 32 | d[i].x) & PACK_KEY_MASK;
                        const bool valid = act && b < num_sigs && b >= cur[i];
                        const uint64_t mm = __ballot(valid && kb == K[i]);
                        const uint64_t me = __ballot(valid && kb > MAX_ENCODED);
                        const uint32_t gm = (uint32_t)(mm >> (G * q)) & ((1u << G) - 1);
                        const uint32_t ge = (uint32_t)(me >> (G * q)) & ((1u << G) - 1);
                        if (act) {
                            const uint32_t ev = gm | ge;
                            if (ev) {
                                const uint32_t first = __builtin_ctz(ev);
                                if (c == first && (gm >> first & 1u)) {
                                    const uint32_t w = 64 * j + NQ * i + q;
                                    lds_rec[wave][w] = d[i];
                                    lds_hit[wave][w] = 1;
                                }
                                live &= ~(1u << i);
                            } else if (round + 1 >= max_lines) {
                                live &= ~(1u << i);
                            } else {
                                cur[i] = line + G >= num_sigs ? 0 : line + G;
                                more = true;
                            }
                        }
                    }
                    if (!__any(more))
                        break;
                }
            }
        }
        wave_lds_sync();

        bool hit[J];
        uint4 pv[J];
#pragma unroll
        for (int j = 0; j < J; j++) {
            hit[j] = lds_hit[wave][64 * j + lane] != 0;
            pv[j] = hit[j] ? lds_rec[wave][64 * j + lane] : make_uint4(0, 0, 0, 0);
        }
        store_tile_hits<J, true>(hit, key, pv, pos, sq, g0, W, lane, hot, cold, hit_mask, nt != 0);
    }
}

/* f(std::integral_constant<int, V>{}) for the V of Vs... that v equals; false,
 * and no call, when it equals none */
template <int... Vs, class F> static bool with_constant(int v, F &&f)
{
    return ((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

template <int J, int G, bool DNA>
static void launch_probe_line(dim3 grid, uint32_t dyn_lds, const ProbeBatch &b, const ProbeTable &t, uint4 *hot,
                              uint4 *cold, uint64_t *hit_mask, bool defer, uint32_t nt, hipStream_t stream)
{
    /* the aligned forms, with the mark test, only over an aligned index
     * (kgx_line_home.h); every other table runs the generic tile, which
     * ignores marks and stays exact.  `defer` picks the aligned form, both
     * compiled: no uniform branch stands in a round */
    auto *kernel = probe_line_kernel<J, G, DNA, false, false, false>;
    if constexpr (G == 4)
        if (line_index_aligned(t.num_sigs, t.home)) {
            if (defer)
                kernel = home_twins_of(t.home) ? probe_line_kernel<J, G, DNA, true, true, true>
                                               : probe_line_kernel<J, G, DNA, true, false, true>;
            else
                kernel = home_twins_of(t.home) ? probe_line_kernel<J, G, DNA, true, true, false>
                                               : probe_line_kernel<J, G, DNA, true, false, false>;
        }
    hipLaunchKernelGGL(kernel, grid, dim3(64 * PROBE_WAVES), dyn_lds, stream, b.bytes, b.n_bytes, b.starts, b.wbase,
                       b.tile_seq, b.n_seq, static_cast<const uint4 *>(t.buckets), t.num_sigs, t.magic(), t.home, hot,
                       cold, hit_mask, nt);
}

template <int J, int MODE>
static void launch_probe_bucket(dim3 grid, const ProbeBatch &b, const ProbeTable &t, const ProbeHits &h,
                                hipStream_t stream)
{
    auto *kernel = t.filter ? probe_kernel<J, MODE, true> : probe_kernel<J, MODE, false>;
    hipLaunchKernelGGL(kernel, grid, dim3(64 * PROBE_WAVES), 0, stream, b.bytes, b.n_bytes, b.starts, b.wbase,
                       b.tile_seq, b.n_seq, t.buckets, t.num_sigs, t.magic(), t.home, t.filter, t.filter_log2_words,
                       h.hot, h.cold, h.hit_mask);
}

static uint32_t probe_workgroups(const ProbeBatch &b) { return (uint32_t)((b.max_tiles + PROBE_WAVES - 1) / PROBE_WAVES); }
/* the line probe strides over tiles when its grid is capped */
static uint32_t line_workgroups(const ProbeBatch &b, const ProbeRun &r)
{
    return r.max_blocks ? std::min<uint32_t>(probe_workgroups(b), r.max_blocks) : probe_workgroups(b);
}

hipError_t launch_probe(const ProbeBatch &b, const ProbeTable &t, const ProbeHits &h, const ProbeRun &r,
                        hipStream_t stream)
{
    constexpr int PACKED16 = KGX_LAYOUT_PACKED16;
    if (b.max_tiles == 0)
        return hipSuccess;
    if (t.home && t.layout != PACKED16)
        return hipErrorInvalidValue; /* line-aligned homes exist for PACKED16 records only */
    int variant = r.variant;
    if (variant == PROBE_AUTO && t.layout == PACKED16 && !t.filter)
        variant = PROBE_LINE;
    if ((variant == PROBE_LINE || variant == PROBE_LINE8) && t.layout == PACKED16 && !t.filter) {
        /* lds_kb > 0: each probe workgroup reserves that much LDS (unused
         * beyond its own ~9 KB), capping the probe at 160 / lds_kb workgroups
         * per CU so that other contexts' kernels find room beside it */
        const uint32_t own_lds = r.defer ? PROBE_LINE_LDS_DEFER : PROBE_LINE_LDS;
        const uint32_t dyn_lds = r.lds_kb * 1024u > own_lds ? r.lds_kb * 1024u - own_lds : 0u;
        const auto line = [&](auto j, auto g) {
            launch_probe_line<decltype(j)::value, decltype(g)::value, false>(
                dim3(line_workgroups(b, r)), dyn_lds, b, t, h.hot, h.cold, h.hit_mask, r.defer, r.nt, stream);
        };
        /* tiles of 64-B lines: J 1-4; of 128-B lines: J 1-2 */
        const bool known = variant == PROBE_LINE8
                               ? with_constant<1, 2>(r.probe_j, [&](auto j) { line(j, std::integral_constant<int, 8>{}); })
                               : with_constant<1, 2, 3, 4>(r.probe_j, [&](auto j) { line(j, std::integral_constant<int, 4>{}); });
        if (known)
            return hipGetLastError();
        /* other tile sizes: the per-bucket kernel below */
    }
    const bool kf = variant == PROBE_AUTO ? t.layout != PACKED16 : variant == PROBE_KEY_FIRST;
    const int mode = t.layout == PACKED16 ? (kf ? MODE_PACKED_KEY_FIRST : MODE_PACKED) : (kf ? MODE_KEY_FIRST : MODE_BUCKET);
    const bool known = with_constant<1, 2, 3, 4, 5, 8>(r.probe_j, [&](auto j) {
        with_constant<MODE_BUCKET, MODE_KEY_FIRST, MODE_PACKED, MODE_PACKED_KEY_FIRST>(mode, [&](auto m) {
            launch_probe_bucket<decltype(j)::value, decltype(m)::value>(dim3(probe_workgroups(b)), b, t, h, stream);
        });
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_probe_dna(const ProbeBatch &b, const ProbeTable &t, const ProbeHits &h, const ProbeRun &r,
                            hipStream_t stream)
{
    if (b.max_tiles == 0)
        return hipSuccess;
    /* J 1-4, 64-B lines; no cold plane, LDS reservation or non-temporal stores */
    const bool known = with_constant<1, 2, 3, 4>(r.probe_j, [&](auto j) {
        launch_probe_line<decltype(j)::value, 4, true>(dim3(line_workgroups(b, r)), 0, b, t, h.hot, nullptr,
                                                       h.hit_mask, r.defer, 0, stream);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace kgx
