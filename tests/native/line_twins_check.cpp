/* The homes behind twin records (csrc/kgx_line_home.h), on the host.
 *   line_twins_check N_LINES
 * checks, for that line count, over the edge keys (0, 20^8 - 1, the twenty
 * homopolymers) and random keys, and over windows of random residue strings:
 *   1. minimizer_home returns what it returned before it was split into
 *      seven_mer_home and a choice (the old formula is restated here);
 *   2. minimizer_home and twin_home are the key's two seven_mer_homes, one
 *      each, and equal where the two 7-mers are;
 *   3. pair_home is one of the key's two seven_mer_homes: the last seven
 *      residues' at an even window index, the first seven's at an odd one;
 *   4. windows g (even) and g + 1 of one sequence have the same pair_home, at
 *      either parity of the sequence's first window.
 * Prints one line per failed check (at most 20) and "ok CHECKS" at the end;
 * exits 1 when any failed. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kgx_line_home.h"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

/* minimizer_home as it was before the split */
static uint64_t old_minimizer_home(uint32_t a, uint32_t b, uint64_t n_lines, uint64_t magic)
{
    const uint32_t ha = kgx::mix32(a), hb = kgx::mix32(b);
    const uint32_t m = ha <= hb ? a : b, hm = ha <= hb ? ha : hb;
    const uint64_t x = (uint64_t)kgx::mix32(m ^ 0x85EBCA6Bu) << 3 | (hm & 7u);
    return kgx::mod_by(x, n_lines, magic);
}

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
    if (n_lines < 1)
        return 2;
    const uint64_t magic = ~0ull / n_lines; /* mod_magic */
    const uint64_t N8 = 25600000000ull, N7 = 1280000000ull;

    std::vector<uint64_t> keys = {0, N8 - 1, 1, N7 - 1, N7, N8 - 20};
    for (uint64_t r = 0; r < 20; r++) { /* homopolymers: both 7-mers equal */
        uint64_t k = 0;
        for (int i = 0; i < 8; i++)
            k = k * 20 + r;
        keys.push_back(k);
    }
    for (int i = 0; i < 200000; i++)
        keys.push_back(rnd() % N8);
    for (uint64_t key : keys) {
        const uint32_t a = (uint32_t)(key / 20), b = (uint32_t)(key % N7);
        const uint64_t sa = kgx::seven_mer_home(a, n_lines, magic), sb = kgx::seven_mer_home(b, n_lines, magic);
        const uint64_t mh = kgx::minimizer_home(a, b, n_lines, magic), th = kgx::twin_home(a, b, n_lines, magic);
        expect(mh == old_minimizer_home(a, b, n_lines, magic), "minimizer_home changed", key, 0);
        expect(mh == kgx::line_home(key, n_lines, magic, kgx::LINE_HOME_MINIMIZER), "line_home", key, 0);
        expect(sa < n_lines && sb < n_lines, "home in range", key, 0);
        expect((mh == sa && th == sb) || (mh == sb && th == sa), "minimizer and twin are the two homes", key, 0);
        expect(a != b || mh == th, "one 7-mer, one home", key, 0);
        expect(sa == kgx::seven_mer_home(a, kgx::mix32(a), n_lines, magic), "seven_mer_home with its hash", key, 0);
        for (uint64_t g = 0; g < 4; g++) {
            const uint64_t ph = kgx::pair_home(a, b, g, n_lines, magic);
            expect(ph == (g & 1 ? sa : sb), "pair_home by parity", key, g);
        }
        expect(kgx::pair_home(a, b, (1ull << 40) + 1, n_lines, magic) == sa, "pair_home of a large index", key, 0);
    }

    /* sequences laid end to end as a batch lays their windows: a sequence of
     * n residues gives n - 7 windows here, and the first window's index in
     * the batch takes both parities because the lengths vary */
    uint64_t g = 0;
    for (int s = 0; s < 400; s++) {
        const uint32_t len = 8 + (uint32_t)(rnd() % 300);
        std::vector<uint32_t> c(len);
        for (auto &x : c)
            x = (uint32_t)(rnd() % (s % 7 == 0 ? 2 : 20)); /* some over two letters: repeats */
        std::vector<uint64_t> home(len - 7);
        for (uint32_t w = 0; w + 8 <= len; w++) {
            uint32_t a, b;
            kgx::seven_mers(&c[w], a, b);
            home[w] = kgx::pair_home(a, b, g + w, n_lines, magic);
        }
        for (uint32_t w = 0; w + 1 < len - 7; w++)
            if (((g + w) & 1) == 0)
                expect(home[w] == home[w + 1], "an even window and the next share their home", s, g + w);
        g += len - 7;
    }
    printf("ok %llu\n", checks);
    return failures ? 1 : 0;
}
