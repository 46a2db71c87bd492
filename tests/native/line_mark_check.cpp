/* line_mark and the home word (csrc/kgx_line_home.h) on the host.  First the
 * home word: shift, home mode and the marks bit round-trip, and the marks bit
 * leaves a key's home bucket where it was (exit 1 otherwise).  Then, for every
 * key on stdin, "mark record bit" per line: its overflow mark, and the record
 * of the line and the bit of that record's last dword that hold it.
 * tests/test_line_mark_native.py compares with a Python restatement. */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "kgx_line_home.h"

int main(int argc, char **argv)
{
    if (argc != 2)
        return 2;
    const uint64_t n_lines = strtoull(argv[1], nullptr, 10);
    if (n_lines < 1)
        return 2;
    const uint64_t magic = ~0ull / n_lines; /* mod_magic */
    for (uint32_t shift : {0u, 2u, 3u, 255u})
        for (uint32_t mode : {0u, 1u, 2u, 255u})
            for (int marks = 0; marks < 2; marks++) {
                const uint32_t w = kgx::home_word(shift, mode, marks != 0);
                if (kgx::home_shift_of(w) != shift || kgx::home_mode_of(w) != mode ||
                    kgx::home_marks_of(w) != (marks != 0))
                    return 1;
                if (!marks && w != kgx::home_word(shift, mode)) /* the two-argument form: no marks */
                    return 1;
            }
    unsigned long long key;
    while (scanf("%llu", &key) == 1) {
        for (uint32_t mode : {kgx::LINE_HOME_MOD, kgx::LINE_HOME_MINIMIZER})
            if (kgx::home_bucket(key, 4 * n_lines, magic, kgx::home_word(2, mode, true)) !=
                kgx::line_home(key, n_lines, magic, mode) * 4)
                return 1;
        const uint32_t g = kgx::line_mark(key);
        if (g >= kgx::LINE_MARKS)
            return 1;
        printf("%u %u %u\n", g, kgx::mark_record(g), kgx::mark_bit_w(g));
    }
    return 0;
}
