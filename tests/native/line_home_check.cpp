/* line_home (csrc/kgx_line_home.h) on the host: for every key on stdin, its
 * home line among argv[1] lines under both home modes, "mod minimizer" per
 * line.  tests/test_line_home_native.py compares with a Python restatement. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "kgx_line_home.h"

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    const uint64_t n_lines = strtoull(argv[1], nullptr, 10);
    if (n_lines < 1)
        return 2;
    const uint64_t magic = ~0ull / n_lines; /* mod_magic */
    unsigned long long key;
    while (scanf("%llu", &key) == 1) {
        const uint64_t h0 = kgx::line_home(key, n_lines, magic, kgx::LINE_HOME_MOD);
        const uint64_t h1 = kgx::line_home(key, n_lines, magic, kgx::LINE_HOME_MINIMIZER);
        /* what the probes compute from the launchers' home word, shift 2 */
        const uint64_t b1 = kgx::home_bucket(key, 4 * n_lines, magic, kgx::home_word(2, kgx::LINE_HOME_MINIMIZER));
        const uint64_t b0 = kgx::home_bucket(key, 4 * n_lines, magic, kgx::home_word(2, kgx::LINE_HOME_MOD));
        if (b1 != 4 * h1 || b0 != 4 * h0 || h0 >= n_lines || h1 >= n_lines)
            return 1;
        printf("%llu %llu\n", (unsigned long long)h0, (unsigned long long)h1);
    }
    return 0;
}
