/*
 * kgx_line_home.h -- the home line of a key in the line index
 * (kgx_image_set_line_index), one function for the builder and every probe.
 * Plain C++ as well as HIP: tests/native/line_home_check.cpp runs it on the
 * host.
 *
 * The index holds, once each, the records the reference's probe reaches
 * first; any deterministic home followed by a linear probe to the key or to
 * an empty bucket returns them, so the home is the index's own choice.
 *
 *   LINE_HOME_MOD        key mod n_lines.
 *   LINE_HOME_MINIMIZER  a key is two overlapping 7-mers, A = key / 20 (its
 *     first seven residues) and B = key mod 20^7 (its last seven); its home
 *     is hashed from whichever of the two has the smaller hash.  Window i's B
 *     is window i + 1's A, so two neighbouring windows of a sequence share
 *     their home line whenever the 7-mer they share is the minimizer of both:
 *     it has the smallest hash of three, probability 1/3, present or absent.
 *     A 7-mer lies in two windows only, so no more than two in a row share.
 *
 * Twin records (HOME_TWINS_BIT, built only over LINE_HOME_MINIMIZER with
 * overflow marks).  The builder inserts every key a second time, walking from
 * the home of its other 7-mer (twin_home), unless both 7-mers are homed on
 * one line; each copy goes to the first empty bucket of its walk, whether or
 * not the walk passes the other copy, so a key with two home lines always
 * has exactly two records.  A key is then found from either of its 7-mers'
 * homes, and the aligned line probe needs no minimum: the window with an even
 * index in its batch starts at the home of its last seven residues and the
 * odd window after it at the home of its first seven, which are the same
 * 7-mer (pair_home), so the two always ask for one line.  A prober that
 * starts at the minimizer home finds the same records as before: the copy
 * that home's walk placed, or the twin where it lies earlier on the chain.
 * The two copies differ in mark bits only.
 *
 * Pairs (HOME_PAIRS_BIT, built only with twin records, over 3 lines or more).
 * A 7-mer S owns a 128-byte block, the aligned lines 2k and 2k + 1 of the
 * n_lines >> 1 blocks, k hashed from S as before: line 2k + 1 is the home of S
 * as a key's first seven residues (role 1), line 2k its home as a key's last
 * seven (role 0).  A key's two homes are those of its two 7-mers, each in its
 * role; they differ in parity, so every key, homopolymers included, has two
 * records.  The even window of a pair starts at line 2k and the odd one after
 * it at 2k + 1: the neighbouring quads of one load instruction read the two
 * halves of one block, a single 128-byte request, and a line collects the
 * keys of one role only, at most 20 instead of 40.  Chains run on as before,
 * line by line and wrapping at n_lines; with n_lines odd the last line is
 * nobody's home and stays in the ring.  The minimizer home, where every other
 * prober starts, is the home of the lower-hashing 7-mer in its role
 * (pairs_minimizer_home).  The home functions under this layout take
 * n_blocks = n_lines >> 1 and its magic, mod_magic(n_blocks): that is the
 * magic the launchers carry for such an index (home_magic_lines).
 *
 * The overflow marks (below) are set per key and per home from the finished
 * index: from each home of a stored key, every line before the first one that
 * holds the key carries the key's mark (lines_mark_kernel walks the index,
 * since a record does not say which home it was inserted from).
 */
#ifndef KGX_LINE_HOME_H
#define KGX_LINE_HOME_H

#include <stdint.h>

#if defined(__HIPCC__)
#define KGX_HD __host__ __device__ __forceinline__
#else
#define KGX_HD inline
#endif

namespace kgx {

constexpr uint32_t LINE_HOME_MOD = 0, LINE_HOME_MINIMIZER = 1;

/* The home word, what the probe launchers take as ProbeTable.home
 * (kgx_internal.h) and the kernels as `home`: bits 0-7 the shift hs (a
 * key's home bucket is home(key) << hs over num_sigs >> hs homes: 0 the
 * reference slots, 2 the 4-bucket lines of the index), bits 8-15 the
 * LINE_HOME_* mode of the image's index (0 where hs is 0), bit 16 set when
 * the index carries overflow marks (line_mark, below), bit 17 set when it
 * holds twin records (above), bit 18 set when a 7-mer's two roles are homed
 * on the halves of a 128-byte block (pairs, above). */
constexpr uint32_t HOME_SHIFT_MASK = 0xFFu, HOME_MODE_SHIFT = 8, HOME_MODE_MASK = 0xFFu, HOME_MARKS_BIT = 1u << 16,
                   HOME_TWINS_BIT = 1u << 17, HOME_PAIRS_BIT = 1u << 18;
KGX_HD uint32_t home_word(uint32_t shift, uint32_t mode, bool marks = false, bool twins = false, bool pairs = false)
{
    return shift | mode << HOME_MODE_SHIFT | (marks ? HOME_MARKS_BIT : 0u) | (twins ? HOME_TWINS_BIT : 0u) |
           (pairs ? HOME_PAIRS_BIT : 0u);
}
KGX_HD uint32_t home_shift_of(uint32_t home) { return home & HOME_SHIFT_MASK; }
KGX_HD uint32_t home_mode_of(uint32_t home) { return home >> HOME_MODE_SHIFT & HOME_MODE_MASK; }
KGX_HD bool home_marks_of(uint32_t home) { return (home & HOME_MARKS_BIT) != 0; }
KGX_HD bool home_twins_of(uint32_t home) { return (home & HOME_TWINS_BIT) != 0; }
KGX_HD bool home_pairs_of(uint32_t home) { return (home & HOME_PAIRS_BIT) != 0; }
/* what the homes of an index of n_lines are taken modulo, and whose magic the
 * launchers carry: the lines, or under pairs the 128-byte blocks */
KGX_HD uint64_t home_magic_lines(uint64_t n_lines, uint32_t home) { return home_pairs_of(home) ? n_lines >> 1 : n_lines; }

/* x % n for x < 2^35, n >= 1, m = floor((2^64-1)/n): the quotient estimate
 * is exact or one short, so one conditional subtraction finishes it */
KGX_HD uint64_t mod_by(uint64_t x, uint64_t n, uint64_t m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint64_t q = __umul64hi(x, m);
#else
    const uint64_t q = (uint64_t)(((unsigned __int128)x * m) >> 64);
#endif
    const uint64_t r = x - q * n;
    return r >= n ? r - n : r;
}

/* a 32-bit bijective mixer (two multiply-xorshift rounds); the added constant
 * keeps 7-mer 0 from hashing to 0, the minimum */
KGX_HD uint32_t mix32(uint32_t x)
{
    x += 0x9E3779B9u;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

/* The two 7-mers of a window from its eight residue codes c[0..7] (each below
 * 20): a = key / 20, b = key mod 20^7, for key the big-endian base-20 number
 * the probes encode as ka * 160000 + kb, ka and kb its two 4-mers.  A probe
 * that has the codes takes the 7-mers from them instead of dividing them back
 * out of the key; both are below 2^31 and every factor is below 2^24. */
KGX_HD void seven_mers(const uint32_t *c, uint32_t &a, uint32_t &b)
{
    const uint32_t ka = ((c[0] * 20 + c[1]) * 20 + c[2]) * 20 + c[3];
    const uint32_t kb = ((c[4] * 20 + c[5]) * 20 + c[6]) * 20 + c[7];
    a = ka * 8000u + (c[4] * 20 + c[5]) * 20 + c[6];
    b = (ka - c[0] * 8000u) * 160000u + kb;
}

/* the home of the 7-mer m, whose hash mix32(m) is hm */
KGX_HD uint64_t seven_mer_home(uint32_t m, uint32_t hm, uint64_t n_lines, uint64_t magic)
{
    /* 35 bits, the most mod_by takes: a second hash of the 7-mer (hm itself
     * leans low where it is a minimum) over three low bits of the first */
    const uint64_t x = (uint64_t)mix32(m ^ 0x85EBCA6Bu) << 3 | (hm & 7u);
    return mod_by(x, n_lines, magic);
}
KGX_HD uint64_t seven_mer_home(uint32_t m, uint64_t n_lines, uint64_t magic)
{
    return seven_mer_home(m, mix32(m), n_lines, magic);
}

/* the minimizer home of the key whose 7-mers are a and b: the home of the one
 * that hashes lower (a on a tie) */
KGX_HD uint64_t minimizer_home(uint32_t a, uint32_t b, uint64_t n_lines, uint64_t magic)
{
    const uint32_t ha = mix32(a), hb = mix32(b);
    return ha <= hb ? seven_mer_home(a, ha, n_lines, magic) : seven_mer_home(b, hb, n_lines, magic);
}

/* the twin home: the home of the other 7-mer (equal to the minimizer home
 * where a == b, and wherever the two 7-mers happen to share a line) */
KGX_HD uint64_t twin_home(uint32_t a, uint32_t b, uint64_t n_lines, uint64_t magic)
{
    const uint32_t ha = mix32(a), hb = mix32(b);
    return ha <= hb ? seven_mer_home(b, hb, n_lines, magic) : seven_mer_home(a, ha, n_lines, magic);
}

/* Where the aligned line probe starts over an index with twin records: window
 * g of a batch (its global window index) at the home of its last seven
 * residues when g is even, of its first seven when g is odd.  Windows g
 * (even) and g + 1 of one sequence share that 7-mer, so they share the line. */
KGX_HD uint64_t pair_home(uint32_t a, uint32_t b, uint64_t g, uint64_t n_lines, uint64_t magic)
{
    return seven_mer_home(g & 1u ? a : b, n_lines, magic);
}

/* Pairs: the home of 7-mer m in role r (1: a key's first seven residues, 0:
 * its last seven), n_blocks = n_lines >> 1 >= 1, magic = mod_magic(n_blocks).
 * The block is hashed as seven_mer_home hashes the line. */
KGX_HD uint64_t pairs_seven_mer_home(uint32_t m, uint32_t hm, uint32_t r, uint64_t n_blocks, uint64_t magic)
{
    return 2 * seven_mer_home(m, hm, n_blocks, magic) + r;
}
KGX_HD uint64_t pairs_seven_mer_home(uint32_t m, uint32_t r, uint64_t n_blocks, uint64_t magic)
{
    return pairs_seven_mer_home(m, mix32(m), r, n_blocks, magic);
}
/* the two homes of the key whose 7-mers are a (first seven) and b (last seven) */
KGX_HD uint64_t pairs_minimizer_home(uint32_t a, uint32_t b, uint64_t n_blocks, uint64_t magic)
{
    const uint32_t ha = mix32(a), hb = mix32(b);
    return ha <= hb ? pairs_seven_mer_home(a, ha, 1u, n_blocks, magic) : pairs_seven_mer_home(b, hb, 0u, n_blocks, magic);
}
KGX_HD uint64_t pairs_twin_home(uint32_t a, uint32_t b, uint64_t n_blocks, uint64_t magic)
{
    const uint32_t ha = mix32(a), hb = mix32(b);
    return ha <= hb ? pairs_seven_mer_home(b, hb, 0u, n_blocks, magic) : pairs_seven_mer_home(a, ha, 1u, n_blocks, magic);
}
/* where window g of a batch starts in the aligned line probe: at its last
 * seven residues' home (line 2k) when g is even, at its first seven's (line
 * 2k + 1) when g is odd; windows g (even) and g + 1 of one sequence share the
 * 7-mer and so the block */
KGX_HD uint64_t pairs_pair_home(uint32_t a, uint32_t b, uint64_t g, uint64_t n_blocks, uint64_t magic)
{
    return pairs_seven_mer_home(g & 1u ? a : b, (uint32_t)(g & 1u), n_blocks, magic);
}

/* The two homes of `key` under the home word of an index of n_lines (its mode,
 * twins and pairs bits), magic = mod_magic(home_magic_lines(n_lines, home)):
 * the builder's and the mark kernel's.  `other` equals `first` for a key
 * with one home line. */
KGX_HD void key_homes(uint64_t key, uint64_t n_lines, uint64_t magic, uint32_t home, uint64_t &first, uint64_t &other)
{
    const uint32_t a = (uint32_t)(key / 20u), b = (uint32_t)(key % 1280000000ull);
    if (home_pairs_of(home)) {
        first = pairs_minimizer_home(a, b, n_lines >> 1, magic);
        other = pairs_twin_home(a, b, n_lines >> 1, magic);
        return;
    }
    const uint32_t mode = home_mode_of(home);
    first = mode == LINE_HOME_MOD ? mod_by(key, n_lines, magic) : minimizer_home(a, b, n_lines, magic);
    other = home_twins_of(home) ? twin_home(a, b, n_lines, magic) : first;
}

/* the home line of `key` (<= 20^8) among n_lines, magic = mod_magic(n_lines) */
KGX_HD uint64_t line_home(uint64_t key, uint64_t n_lines, uint64_t magic, uint32_t mode)
{
    if (mode == LINE_HOME_MOD)
        return mod_by(key, n_lines, magic);
    const uint32_t a = (uint32_t)(key / 20u), b = (uint32_t)(key % 1280000000ull); /* 7-mers: below 2^31 */
    return minimizer_home(a, b, n_lines, magic);
}

/* the same home for a caller that holds the key's 7-mers (seven_mers): no
 * 64-bit division (the key is 20 a + the last residue, b mod 20) */
KGX_HD uint64_t line_home_7mers(uint32_t a, uint32_t b, uint64_t n_lines, uint64_t magic, uint32_t mode)
{
    if (mode == LINE_HOME_MOD)
        return mod_by((uint64_t)a * 20u + b % 20u, n_lines, magic);
    return minimizer_home(a, b, n_lines, magic);
}

/* Whether a probe table of num_sigs buckets under the launchers' home word
 * is an aligned index: whole 4-record lines, line-aligned homes, overflow
 * marks (below), and few enough lines that a line number, and the n_lines + 2
 * lines a chain may visit, fit 32 bits.  The line probe's aligned slice body
 * holds for exactly these tables; every other one runs the generic kernel. */
KGX_HD bool line_index_aligned(uint64_t num_sigs, uint32_t home)
{
    return home_marks_of(home) && home_shift_of(home) == 2 && num_sigs >= 4 && num_sigs % 4 == 0 &&
           num_sigs / 4 <= 0xFFFFFFFFull - 2;
}

/* the home bucket of `key` in a probe table of num_sigs buckets; `home` as
 * above, magic = mod_magic(home_magic_lines(num_sigs >> hs, home)) */
KGX_HD uint64_t home_bucket(uint64_t key, uint64_t num_sigs, uint64_t magic, uint32_t home)
{
    const uint32_t hs = home_shift_of(home);
    if (home_pairs_of(home)) {
        const uint32_t a = (uint32_t)(key / 20u), b = (uint32_t)(key % 1280000000ull);
        return pairs_minimizer_home(a, b, num_sigs >> hs >> 1, magic) << hs;
    }
    return line_home(key, num_sigs >> hs, magic, home_mode_of(home)) << hs;
}

/* Overflow marks.  A PACKED16 record leaves bits 60-63 of its second word
 * unused, so the four records of an index line carry 16 spare bits.  Bit
 * line_mark(K) of line L is set if and only if some stored key with that mark
 * visited L during its insertion and was placed in a later line (only full
 * lines are passed, so only full lines carry marks).  A probe that has
 * searched a full line for K without finding it, and finds K's mark clear
 * there, knows K is not stored: a stored K not in L whose chain visits L left
 * L and set the bit.
 *
 * The mark is a hash of the whole key, independent of the home hash: the up
 * to 40 keys that share a minimizer differ in one end residue only, and they
 * spread over the 16 values.  Mark g lives in record g >> 2 of the line, bit
 * 60 + (g & 3) of its second word (bit 28 + (g & 3) of its last dword). */
constexpr uint32_t LINE_MARKS = 16;
constexpr uint64_t MARK_BITS_HI = 0xFull << 60; /* a record's share of its line's marks */
constexpr uint32_t MARK_BITS_W = 0xFu << 28;    /* the same in the record's last dword */
KGX_HD uint32_t line_mark(uint64_t key)
{
    return mix32(((uint32_t)key ^ 0x27D4EB2Fu) + (uint32_t)(key >> 32) * 0xC2B2AE35u) >> 28;
}
KGX_HD uint32_t mark_record(uint32_t g) { return g >> 2; }
KGX_HD uint32_t mark_bit_w(uint32_t g) { return 28u + (g & 3u); }

}  // namespace kgx

#endif
