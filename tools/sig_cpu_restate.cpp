/*
 * sig_cpu_restate.cpp -- the signature selection rules on one
 * CPU thread: enumerate tuples, std::sort them by (key, n), walk the sets.
 * The baseline tools/bench_signatures.py prints beside the device's time; it
 * builds this file into a shared library itself.
 */
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <vector>

namespace {

struct Tuple {
    uint64_t key;
    uint32_t n;
    uint32_t seq;
};

bool letter_ok(uint8_t c)
{
    static const bool *tab = [] {
        static bool t[256] = {};
        for (const char *p = "ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy"; *p; p++)
            t[(uint8_t)*p] = true;
        return t;
    }();
    return tab[c];
}

}  // namespace

/* out: n_tuples, n_sets, n_kept, NSF, sum of medians, sum of n_best, then
 * out_wt_sum = the weights summed in double.  Returns the seconds taken. */
extern "C" double sig_cpu_select(const uint8_t *res, const uint64_t *off, const int32_t *fn, uint32_t n_seq,
                                 uint32_t n_functions, uint64_t *out, double *out_wt_sum)
{
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> NF(n_functions, 0);
    std::vector<Tuple> tuples;
    for (uint32_t s = 0; s < n_seq; s++) {
        if (fn[s] < 0)
            continue;
        NF[fn[s]]++;
        const uint64_t b = off[s], len = off[s + 1] - b;
        for (uint64_t p = 0; p + 8 <= len; p++) {
            uint64_t key = 0;
            bool ok = true;
            for (int j = 0; j < 8 && ok; j++) {
                ok = letter_ok(res[b + p + j]);
                key = key << 8 | res[b + p + j];
            }
            if (ok)
                tuples.push_back({key, (uint32_t)(len - p), s});
        }
    }
    std::sort(tuples.begin(), tuples.end(),
              [](const Tuple &a, const Tuple &b) { return a.key != b.key ? a.key < b.key : a.n < b.n; });
    struct Kept {
        int32_t best;
        uint32_t count, n_best, median;
    };
    std::vector<Kept> kept;
    std::vector<uint8_t> has_sig(n_seq, 0);
    std::vector<uint32_t> votes(n_functions, 0);
    uint64_t n_sets = 0;
    for (size_t i = 0; i < tuples.size();) {
        size_t j = i;
        while (j < tuples.size() && tuples[j].key == tuples[i].key)
            j++;
        n_sets++;
        int32_t best = -1;
        uint32_t n_best = 0;
        for (size_t k = i; k < j; k++) {
            const int32_t f = fn[tuples[k].seq];
            if (++votes[f] > n_best) {
                n_best = votes[f];
                best = f;
            }
        }
        for (size_t k = i; k < j; k++)
            votes[fn[tuples[k].seq]] = 0;
        const uint32_t count = (uint32_t)(j - i);
        const float thresh = float(count) * 0.8;
        if (!((float)n_best < thresh)) {
            kept.push_back({best, count, n_best, tuples[i + count / 2].n});
            for (size_t k = i; k < j; k++)
                has_sig[tuples[k].seq] = 1;
        }
        i = j;
    }
    uint64_t nsf = 0;
    for (uint8_t h : has_sig)
        nsf += h;
    uint64_t med_sum = 0, best_sum = 0;
    double wt_sum = 0;
    const float NSF = (float)nsf, KS = (float)kept.size();
    for (const Kept &k : kept) {
        const float NSi = (float)k.count, NFj = (float)NF[k.best], NSiFj = (float)k.n_best;
        const float w = (float)(std::log((NSiFj + 1.0) / (NSi - NSiFj + 1.0)) +
                                std::log((double)((NSF - NFj + KS) / (NFj + KS))));
        wt_sum += w;
        med_sum += k.median;
        best_sum += k.n_best;
    }
    out[0] = tuples.size();
    out[1] = n_sets;
    out[2] = kept.size();
    out[3] = nsf;
    out[4] = med_sum;
    out[5] = best_sum;
    *out_wt_sum = wt_sum;
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
