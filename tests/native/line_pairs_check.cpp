/* The homes of the pairs layout (HOME_PAIRS_BIT, csrc/kgx_line_home.h), on the
 * host.
 *   line_pairs_check N_LINES      (N_LINES >= 3)
 * checks, for that line count, over the edge keys (0, 20^8 - 1, the twenty
 * homopolymers) and random keys, and over windows of random residue strings:
 *   1. a key's two homes (key_homes under the pairs bit, pairs_minimizer_home
 *      and pairs_twin_home) are its 7-mers' homes in their roles: the first
 *      seven residues' in role 1, the last seven's in role 0, each
 *      2 * mod_by(x, n_lines >> 1) + role with x restated here;
 *   2. the two differ (in parity), homopolymers included, and both are below
 *      2 * (n_lines >> 1), so the last line of an odd n_lines is nobody's home;
 *   3. the minimizer home, and home_bucket / 4 under the bit, is the home of
 *      the lower-hashing 7-mer in its role, so one of the two;
 *   4. windows g (even) and g + 1 of one sequence start (pairs_pair_home, and
 *      the probe's (h << sp) | (lane & sp) restated here) at lines 2k and
 *      2k + 1 of one block, at either parity of the sequence's first window;
 *   5. without the bit home_bucket, key_homes, line_home and line_home_7mers
 *      return what they returned (the formulas of the index without pairs
 *      restated here).
 * Prints one line per failed check (at most 20) and "ok CHECKS" at the end;
 * exits 1 when any failed. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kgx_line_home.h"

static uint64_t rng_state = 0x13198A2E03707344ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

/* today's 35-bit value of a 7-mer, restated */
static uint64_t x_of(uint32_t m) { return (uint64_t)kgx::mix32(m ^ 0x85EBCA6Bu) << 3 | (kgx::mix32(m) & 7u); }
/* plain remainder: the reference for mod_by */
static uint64_t role_home(uint32_t m, uint32_t r, uint64_t n_blocks) { return 2 * (x_of(m) % n_blocks) + r; }

static int failures = 0;
static unsigned long long checks = 0;
static void expect(bool ok, const char *what, unsigned long long key, unsigned long long g)
{
    checks++;
    if (!ok && failures++ < 20)
        printf("FAILED %s: key %llu window %llu\n", what, key, g);
}

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    const uint64_t n_lines = strtoull(argv[1], nullptr, 10);
    if (n_lines < 3)
        return 2;
    const uint64_t n_blocks = n_lines >> 1;
    const uint64_t magic = ~0ull / n_blocks, old_magic = ~0ull / n_lines; /* mod_magic */
    const uint64_t N8 = 25600000000ull, N7 = 1280000000ull;
    const uint32_t MINI = kgx::LINE_HOME_MINIMIZER;
    const uint32_t hw_pairs = kgx::home_word(2u, MINI, true, true, true);
    const uint32_t hw_twins = kgx::home_word(2u, MINI, true, true), hw_marks = kgx::home_word(2u, MINI, true);
    const uint32_t hw_mod = kgx::home_word(2u, kgx::LINE_HOME_MOD);
    expect(kgx::home_pairs_of(hw_pairs) && !kgx::home_pairs_of(hw_twins) && hw_pairs == (hw_twins | 1u << 18),
           "the pairs bit is bit 18", 0, 0);
    expect(kgx::HOME_PAIRS_BIT == 1u << 18, "HOME_PAIRS_BIT", 0, 0);
    expect(kgx::home_magic_lines(n_lines, hw_pairs) == n_blocks && kgx::home_magic_lines(n_lines, hw_twins) == n_lines,
           "home_magic_lines", 0, 0);
    expect(kgx::home_word(2u, MINI, true, true) == (2u | 1u << 8 | 1u << 16 | 1u << 17), "home_word without pairs", 0, 0);

    std::vector<uint64_t> keys = {0, N8 - 1, 1, N7 - 1, N7, N8 - 20};
    for (uint64_t r = 0; r < 20; r++) { /* homopolymers: both 7-mers equal */
        uint64_t k = 0;
        for (int i = 0; i < 8; i++)
            k = k * 20 + r;
        keys.push_back(k);
    }
    for (int i = 0; i < 100000; i++)
        keys.push_back(rnd() % N8);
    for (uint64_t key : keys) {
        const uint32_t a = (uint32_t)(key / 20), b = (uint32_t)(key % N7);
        const uint64_t ha = role_home(a, 1, n_blocks), hb = role_home(b, 0, n_blocks);
        expect(kgx::pairs_seven_mer_home(a, 1u, n_blocks, magic) == ha, "first seven in role 1", key, 0);
        expect(kgx::pairs_seven_mer_home(b, 0u, n_blocks, magic) == hb, "last seven in role 0", key, 0);
        expect(ha != hb, "the two homes differ", key, 0);
        expect(ha < 2 * n_blocks && hb < 2 * n_blocks && ha < n_lines && hb < n_lines, "homes in range", key, 0);
        const uint64_t mh = kgx::pairs_minimizer_home(a, b, n_blocks, magic);
        const uint64_t th = kgx::pairs_twin_home(a, b, n_blocks, magic);
        expect((mh == ha && th == hb) || (mh == hb && th == ha), "minimizer and twin are the two homes", key, 0);
        expect(mh == (kgx::mix32(a) <= kgx::mix32(b) ? ha : hb), "the minimizer home is the lower hash's", key, 0);
        uint64_t f, o;
        kgx::key_homes(key, n_lines, magic, hw_pairs, f, o);
        expect(f == mh && o == th, "key_homes under pairs", key, 0);
        expect(kgx::home_bucket(key, 4 * n_lines, magic, hw_pairs) == 4 * mh, "home_bucket under pairs", key, 0);
        for (uint64_t g = 0; g < 4; g++)
            expect(kgx::pairs_pair_home(a, b, g, n_blocks, magic) == (g & 1 ? ha : hb), "pairs_pair_home by parity", key, g);

        /* without the bit: as it was */
        const uint64_t sa = x_of(a) % n_lines, sb = x_of(b) % n_lines;
        const bool a_low = kgx::mix32(a) <= kgx::mix32(b);
        const uint64_t omh = a_low ? sa : sb, oth = a_low ? sb : sa;
        expect(kgx::seven_mer_home(a, n_lines, old_magic) == sa && kgx::seven_mer_home(b, n_lines, old_magic) == sb,
               "seven_mer_home", key, 0);
        expect(kgx::minimizer_home(a, b, n_lines, old_magic) == omh && kgx::twin_home(a, b, n_lines, old_magic) == oth,
               "minimizer_home and twin_home", key, 0);
        expect(kgx::line_home(key, n_lines, old_magic, MINI) == omh, "line_home", key, 0);
        expect(kgx::line_home(key, n_lines, old_magic, kgx::LINE_HOME_MOD) == key % n_lines, "line_home mod", key, 0);
        expect(kgx::line_home_7mers(a, b, n_lines, old_magic, MINI) == omh, "line_home_7mers", key, 0);
        expect(kgx::line_home_7mers(a, b, n_lines, old_magic, kgx::LINE_HOME_MOD) == key % n_lines, "line_home_7mers mod",
               key, 0);
        expect(kgx::home_bucket(key, 4 * n_lines, old_magic, hw_twins) == 4 * omh, "home_bucket twins", key, 0);
        expect(kgx::home_bucket(key, 4 * n_lines, old_magic, hw_marks) == 4 * omh, "home_bucket marks", key, 0);
        expect(kgx::home_bucket(key, 4 * n_lines, old_magic, hw_mod) == 4 * (key % n_lines), "home_bucket mod", key, 0);
        expect(kgx::home_bucket(key, n_lines, old_magic, 0u) == key % n_lines, "home_bucket reference slots", key, 0);
        kgx::key_homes(key, n_lines, old_magic, hw_twins, f, o);
        expect(f == omh && o == oth, "key_homes twins", key, 0);
        kgx::key_homes(key, n_lines, old_magic, hw_marks, f, o);
        expect(f == omh && o == omh, "key_homes without twins", key, 0);
        kgx::key_homes(key, n_lines, old_magic, hw_mod, f, o);
        expect(f == key % n_lines && o == f, "key_homes mod", key, 0);
        for (uint64_t g = 0; g < 2; g++)
            expect(kgx::pair_home(a, b, g, n_lines, old_magic) == (g & 1 ? sa : sb), "pair_home", key, g);
    }

    /* sequences laid end to end as a batch lays their windows: a sequence of
     * n residues gives n - 7 windows, and the first window's index in the
     * batch takes both parities because the lengths vary */
    uint64_t g = 0;
    unsigned long long firsts[2] = {0, 0};
    for (int s = 0; s < 300; s++) {
        const uint32_t len = 8 + (uint32_t)(rnd() % 40);
        std::vector<uint32_t> c(len);
        for (auto &x : c)
            x = (uint32_t)(rnd() % (s % 7 == 0 ? 2 : 20)); /* some over two letters: repeats */
        std::vector<uint64_t> home(len - 7);
        for (uint32_t w = 0; w + 8 <= len; w++) {
            uint32_t a, b;
            kgx::seven_mers(&c[w], a, b);
            home[w] = kgx::pairs_pair_home(a, b, g + w, n_blocks, magic);
            /* the aligned probe's form: sp = 1, the lane's parity is g's */
            const uint32_t sp = 1, lane = (uint32_t)((g + w) & 63);
            const uint64_t probe = kgx::pair_home(a, b, lane, n_lines >> sp, magic) << sp | (lane & sp);
            expect(probe == home[w], "the probe's start line", s, g + w);
            uint64_t f, o;
            kgx::key_homes(((uint64_t)a) * 20 + b % 20, n_lines, magic, hw_pairs, f, o);
            expect(home[w] == f || home[w] == o, "a window starts at a home of its key", s, g + w);
        }
        firsts[g & 1]++;
        for (uint32_t w = 0; w + 1 < len - 7; w++)
            if (((g + w) & 1) == 0) {
                expect((home[w] & 1) == 0 && home[w + 1] == home[w] + 1, "an even window and the next: lines 2k and 2k + 1",
                       s, g + w);
                expect(home[w + 1] < n_lines, "the block inside the table", s, g + w);
            }
        g += len - 7;
    }
    expect(firsts[0] > 50 && firsts[1] > 50, "both parities of a sequence's first window", 0, 0);
    printf("ok %llu\n", checks);
    return failures ? 1 : 0;
}
