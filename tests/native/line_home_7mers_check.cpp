/* The home of a key from its two 7-mers (csrc/kgx_line_home.h), on the host.
 *   line_home_7mers_check N_LINES < keys
 * For every key on stdin: its eight base-20 codes, seven_mers over them, and
 * line_home_7mers of the result under both modes; prints "a b mod minimizer"
 * per line, and exits 1 where seven_mers disagrees with the two divisions it
 * replaces or a home with line_home of the key.
 *   line_home_7mers_check aligned NUM_SIGS SHIFT MODE MARKS
 * prints 1 or 0: line_index_aligned, the line probe launcher's choice of the
 * aligned slice body. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "kgx_line_home.h"

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "aligned")) {
        const uint64_t num_sigs = strtoull(argv[2], nullptr, 10);
        const uint32_t home = kgx::home_word((uint32_t)atoi(argv[3]), (uint32_t)atoi(argv[4]), atoi(argv[5]) != 0);
        printf("%d\n", kgx::line_index_aligned(num_sigs, home) ? 1 : 0);
        return 0;
    }
    if (argc != 2)
        return 2;
    const uint64_t n_lines = strtoull(argv[1], nullptr, 10);
    if (n_lines < 1)
        return 2;
    const uint64_t magic = ~0ull / n_lines; /* mod_magic */
    unsigned long long key;
    while (scanf("%llu", &key) == 1) {
        uint32_t c[8];
        uint64_t k = key;
        for (int i = 7; i >= 0; i--) {
            c[i] = (uint32_t)(k % 20);
            k /= 20;
        }
        if (k)
            return 2; /* not a key */
        uint32_t a, b;
        kgx::seven_mers(c, a, b);
        if (a != key / 20 || b != key % 1280000000ull)
            return 1;
        const uint64_t h0 = kgx::line_home_7mers(a, b, n_lines, magic, kgx::LINE_HOME_MOD);
        const uint64_t h1 = kgx::line_home_7mers(a, b, n_lines, magic, kgx::LINE_HOME_MINIMIZER);
        if (h0 != kgx::line_home(key, n_lines, magic, kgx::LINE_HOME_MOD) ||
            h1 != kgx::line_home(key, n_lines, magic, kgx::LINE_HOME_MINIMIZER) ||
            h1 != kgx::minimizer_home(a, b, n_lines, magic))
            return 1;
        printf("%u %u %llu %llu\n", a, b, (unsigned long long)h0, (unsigned long long)h1);
    }
    return 0;
}
