/*
 * kguts_impl.h -- what the facade's source files (kguts_hip.cpp,
 * kguts_mapping.cpp, kguts_lookup.cpp, kguts_fq.cpp) share and kguts_hip.h
 * does not export.  Not included by kguts_hip.h.
 */
#pragma once

#include <charconv>
#include <chrono>
#include <cmath>
#include <string>

#include "kguts_hip.h"

namespace kgx {

int fail(int code, const std::string &msg); /* kgx_runtime.cpp: sets kgx_last_error() */

inline constexpr char kResidues[21] = "ACDEFGHIKLMNPQRSTVWY";

/* Error(rc, "what: <kgx_strerror> (<kgx_last_error>)") */
[[noreturn]] void throw_last(int rc, const std::string &what);

inline uint64_t now_ns()
{
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

/* iostream's default formatting of the numbers in the handler lines
 * (format_call / format_hit / format_otu_stats, kguts.cc:939-973) */
inline void append_u64(std::string &out, unsigned long long v)
{
    char b[24];
    auto r = std::to_chars(b, b + sizeof b, v);
    out.append(b, r.ptr);
}

inline void append_i64(std::string &out, long long v)
{
    char b[24];
    auto r = std::to_chars(b, b + sizeof b, v);
    out.append(b, r.ptr);
}

/* operator<<(float) with precision 6 and no floatfield is "%.*g" of the
 * value widened to double (libstdc++ num_put::_M_insert_float); to_chars in
 * general format with a precision is specified as printf's %.6g, at a quarter
 * of snprintf's cost.  Integral values below 1e6 in magnitude -- the scores
 * (counts) and the zeros of most output lines -- print as %.6g prints them,
 * their digits (and "-0" for negative zero), without the float formatter.
 * kgx_format_g6 exports it; tests/test_abi_host.py checks it against
 * printf's %.6g. */
inline size_t format_g6(char *b, size_t cap, float v)
{
    const double d = (double)v;
    if (d == 0.0) {
        if (std::signbit(d)) {
            b[0] = '-';
            b[1] = '0';
            return 2;
        }
        b[0] = '0';
        return 1;
    }
    if (d > -1e6 && d < 1e6 && d == (double)(long long)d)
        return (size_t)(std::to_chars(b, b + cap, (long long)d).ptr - b);
    /* 1e-4 <= |v| < 1e6 (the scores): with 10^e <= |v| < 10^(e+1), |v| *
     * 10^(5-e) is exact in a double (24 + at most 21 bits), so rounding it
     * to an integer (nearbyint: to nearest, ties to even) gives printf's six
     * significant digits; fixed notation, trailing zeros dropped */
    static const double p10[] = {1e-4, 1e-3, 1e-2, 1e-1, 1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9};
    const double a = std::fabs(d);
    if (cap >= 16 && a >= 1e-4 && a < 1e6) {
        int e = 5;
        while (a < p10[e + 4])
            e--;
        long long r = (long long)std::nearbyint(a * p10[5 - e + 4]);
        if (r == 1000000) { /* rounded up to 10^(e+1) */
            if (e == 5)
                return (size_t)(std::to_chars(b, b + cap, d, std::chars_format::general, 6).ptr - b);
            r = 100000;
            e++;
        }
        char dig[6];
        for (int i = 5; i >= 0; i--, r /= 10)
            dig[i] = (char)('0' + r % 10);
        size_t n = 0;
        if (d < 0)
            b[n++] = '-';
        int last = 5; /* the last significant digit kept */
        while (last > 0 && last > e && dig[last] == '0')
            last--;
        if (e >= 0) {
            for (int i = 0; i <= e; i++)
                b[n++] = dig[i];
            if (last > e) {
                b[n++] = '.';
                for (int i = e + 1; i <= last; i++)
                    b[n++] = dig[i];
            }
        } else {
            b[n++] = '0';
            b[n++] = '.';
            for (int i = 0; i < -e - 1; i++)
                b[n++] = '0';
            for (int i = 0; i <= last; i++)
                b[n++] = dig[i];
        }
        return n;
    }
    return (size_t)(std::to_chars(b, b + cap, d, std::chars_format::general, 6).ptr - b);
}

inline void append_f32(std::string &out, float v)
{
    char b[48];
    out.append(b, format_g6(b, sizeof b, v));
}

/* a sequence's rollup rows into a score map as the reference's operator[]
 * calls leave it (family_mapper.cc:287-312, lookup_request.cc:446-482): the
 * ids in first-touch order, which is the rows' order.  The map is not
 * cleared: the callers differ on when they clear. */
template <typename Map>
inline void fill_scores(Map &m, const kgx_rollup_row *rows, size_t n)
{
    for (size_t j = 0; j < n; j++) {
        auto &s = m[rows[j].id];
        s.hit_count = rows[j].hit_count;
        s.hit_total = rows[j].hit_total;
        s.weighted_total = rows[j].weighted_total;
    }
}

}  // namespace kgx
