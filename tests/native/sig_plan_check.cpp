/* The pass planner of signature selection (csrc/kgx_sig_plan.h) over small
 * corpora, with a counter that walks sorted keys on the CPU where the device
 * runs sig_count_kernel.  For budgets from "everything" down to the largest
 * set: the passes are ascending, disjoint and cover every key; none holds
 * more than the budget; each count is the direct count; two neighbours
 * together exceed the budget.  One below the largest set is KGX_ERANGE and
 * names the k-mer.  Also the rank table and the automatic budget.  Prints
 * "ok <checks>"; any failure prints a line and exits 1. */
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "kgx_sig_plan.h"

using namespace kgx;

static long g_checks = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        g_checks++;                                   \
        if (!(cond)) {                                \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                 \
            std::printf("\n");                        \
            std::exit(1);                             \
        }                                             \
    } while (0)

/* the sorted keys of every window of 8 letters, as the emit kernel forms them */
static std::vector<uint64_t> keys_of(const std::vector<std::string> &seqs)
{
    uint8_t rank[256];
    sig_rank_table(rank);
    std::vector<uint64_t> keys;
    for (const std::string &s : seqs)
        for (size_t p = 0; p + 8 <= s.size(); p++) {
            uint64_t k = 0;
            bool ok = true;
            for (int j = 0; j < 8; j++) {
                const uint8_t c = (uint8_t)s[p + j];
                ok = ok && rank[c] != kSigNoRank;
                k = k << 8 | c;
            }
            if (ok)
                keys.push_back(k);
        }
    std::sort(keys.begin(), keys.end());
    return keys;
}

static SigCounter counter_over(const std::vector<uint64_t> &keys)
{
    return [&keys](uint64_t prefix, int d, uint64_t *counts) {
        uint8_t rank[256];
        sig_rank_table(rank);
        const int rest = 64 - 8 * d;
        for (uint64_t k : keys) {
            if (d && (k ^ prefix) >> rest)
                continue;
            counts[rank[(k >> (rest - 8)) & 0xFF] * kSigRanks + rank[(k >> (rest - 16)) & 0xFF]]++;
        }
        return KGX_OK;
    };
}

static uint64_t count_in(const std::vector<uint64_t> &keys, uint64_t lo, uint64_t hi)
{
    return (uint64_t)(std::lower_bound(keys.begin(), keys.end(), hi) - std::lower_bound(keys.begin(), keys.end(), lo));
}

static std::string kmer_of(uint64_t k)
{
    std::string s(8, '?');
    for (int j = 0; j < 8; j++)
        s[j] = (char)(k >> (8 * (7 - j)));
    return s;
}

static void check_corpus(const char *name, const std::vector<std::string> &seqs)
{
    const std::vector<uint64_t> keys = keys_of(seqs);
    const uint64_t T = keys.size();
    CHECK(T > 0, "%s", name);
    /* the largest set, and the first key (ascending) that holds it */
    uint64_t M = 0, m_key = 0;
    for (size_t i = 0; i < keys.size();) {
        size_t j = i;
        while (j < keys.size() && keys[j] == keys[i])
            j++;
        if (j - i > M) {
            M = j - i;
            m_key = keys[i];
        }
        i = j;
    }
    std::set<uint64_t> budgets = {T + 5, T, T - 1, T / 2, T / 3, T / 7, T / 20, T / 100, 2 * M, M + 1, M};
    for (uint64_t B : budgets) {
        if (B < M)
            continue;
        SigPlanner planner(B, counter_over(keys));
        std::vector<SigPass> passes;
        const int rc = planner.plan(&passes);
        CHECK(rc == KGX_OK, "%s B=%llu rc=%d %s", name, (unsigned long long)B, rc, planner.error().c_str());
        uint64_t sum = 0;
        for (size_t i = 0; i < passes.size(); i++) {
            const SigPass &p = passes[i];
            CHECK(p.lo_key < p.hi_key, "%s B=%llu pass %zu", name, (unsigned long long)B, i);
            CHECK(i == 0 || passes[i - 1].hi_key <= p.lo_key, "%s B=%llu pass %zu overlaps", name,
                  (unsigned long long)B, i);
            CHECK(p.n_tuples > 0 && p.n_tuples <= B, "%s B=%llu pass %zu holds %llu", name, (unsigned long long)B, i,
                  (unsigned long long)p.n_tuples);
            CHECK(count_in(keys, p.lo_key, p.hi_key) == p.n_tuples, "%s B=%llu pass %zu: %llu planned, %llu there", name,
                  (unsigned long long)B, i, (unsigned long long)p.n_tuples,
                  (unsigned long long)count_in(keys, p.lo_key, p.hi_key));
            CHECK(i == 0 || passes[i - 1].n_tuples + p.n_tuples > B, "%s B=%llu passes %zu and %zu fit one", name,
                  (unsigned long long)B, i - 1, i);
            sum += p.n_tuples;
        }
        /* the counts are exact and the passes disjoint: summing to T is covering every key */
        CHECK(sum == T, "%s B=%llu covers %llu of %llu", name, (unsigned long long)B, (unsigned long long)sum,
              (unsigned long long)T);
        CHECK(passes.size() <= 2 * T / B + 1 && passes.size() >= (T + B - 1) / B, "%s B=%llu: %zu passes", name,
              (unsigned long long)B, passes.size());
        if (B >= T)
            CHECK(passes.size() == 1 && planner.count_calls() == 1, "%s B=%llu: %zu passes", name,
                  (unsigned long long)B, passes.size());
    }
    if (M > 1) {
        SigPlanner planner(M - 1, counter_over(keys));
        std::vector<SigPass> passes;
        const int rc = planner.plan(&passes);
        CHECK(rc == KGX_ERANGE, "%s B=M-1 rc=%d", name, rc);
        CHECK(planner.error().find("k-mer " + kmer_of(m_key) + " ") != std::string::npos, "%s: %s", name,
              planner.error().c_str());
        CHECK(planner.error().find(" " + std::to_string(M) + " tuples") != std::string::npos, "%s: %s", name,
              planner.error().c_str());
    }
    /* a counter's error ends the planning */
    SigPlanner broken(1, [](uint64_t, int, uint64_t *) { return KGX_EDEVICE; });
    std::vector<SigPass> none;
    CHECK(broken.plan(&none) == KGX_EDEVICE && none.empty(), "%s", name);
    std::printf("# %s: %llu tuples, largest set %llu (%s)\n", name, (unsigned long long)T, (unsigned long long)M,
                kmer_of(m_key).c_str());
}

static std::string random_seq(std::mt19937_64 &rng, const std::string &alphabet, size_t n)
{
    std::string s(n, 'A');
    for (char &c : s)
        c = alphabet[rng() % alphabet.size()];
    return s;
}

static void check_rank_table()
{
    uint8_t rank[256];
    sig_rank_table(rank);
    int letters = 0, last = -1;
    for (int c = 0; c < 256; c++) {
        if (rank[c] == kSigNoRank)
            continue;
        CHECK(rank[c] == letters && c > last, "byte %d rank %d", c, rank[c]); /* ascending bytes, ascending ranks */
        CHECK(kSigLetters[rank[c]] == (char)c, "byte %d", c);
        last = c;
        letters++;
    }
    CHECK(letters == (int)kSigRanks && sizeof(kSigLetters) == kSigRanks + 1, "%d letters", letters);
    CHECK(rank['A'] == 0 && rank['Y'] == 19 && rank['a'] == 20 && rank['y'] == 39, "ends");
    CHECK(rank['B'] == kSigNoRank && rank['X'] == kSigNoRank && rank['*'] == kSigNoRank && rank[0] == kSigNoRank &&
              rank['b'] == kSigNoRank,
          "others");
    CHECK(sig_bin_key(0, 0, 0) == 0x4141000000000000ull && sig_bin_key(0x4141000000000000ull, 2, 41) == 0x4141434300000000ull,
          "bin keys");
}

static void check_budget()
{
    const uint64_t windows[] = {0, 1, 1000, 1ull << 20, 1ull << 31, 1ull << 33, 1ull << 36, 1ull << 40};
    for (uint64_t W : windows) {
        uint64_t before = 0;
        for (uint64_t f = 0; f < (400ull << 30); f = f < (1ull << 20) ? f + 4099 : f + f / 64 + 12345) {
            const uint64_t B = sig_auto_budget(f, W);
            CHECK(B >= 1 && B <= kSigMaxPassTuples, "free %llu", (unsigned long long)f);
            CHECK(B >= before, "not monotone at free %llu, %llu windows", (unsigned long long)f, (unsigned long long)W);
            before = B;
            const uint64_t avail = f > kSigFixedBytes ? f - kSigFixedBytes : 0;
            /* one pass with its records, where that fits and the int allows it */
            if (avail >= W * (kSigPassBytesPerTuple + kSigRecordBytes) && W <= kSigMaxPassTuples)
                CHECK(B >= W, "free %llu, %llu windows: budget %llu", (unsigned long long)f, (unsigned long long)W,
                      (unsigned long long)B);
            /* several passes: the largest and a record per window fit, where the worst case is reserved */
            if (B < W && B > 1 && avail / 2 >= W * kSigRecordBytes)
                CHECK(B * kSigPassBytesPerTuple + W * kSigRecordBytes <= avail, "free %llu, %llu windows",
                      (unsigned long long)f, (unsigned long long)W);
            /* in every case the passes fit beside half of the memory */
            if (B > 1)
                CHECK(B * kSigPassBytesPerTuple <= std::max(avail, (uint64_t)1), "free %llu", (unsigned long long)f);
        }
    }
    CHECK(sig_auto_budget(~0ull, ~0ull) <= kSigMaxPassTuples && sig_auto_budget(0, 0) == 1, "extremes");
}

int main()
{
    check_rank_table();
    check_budget();
    std::mt19937_64 rng(0x51671);
    const std::string upper = "ACDEFGHIKLMNPQRSTVWY", lower = "acdefghiklmnpqrstvwy";

    std::vector<std::string> c20, c4, both, one;
    for (int i = 0; i < 200; i++)
        c20.push_back(random_seq(rng, upper, 20 + rng() % 120));
    check_corpus("20 letters", c20);
    for (int i = 0; i < 300; i++) /* 16 bins at depth 0: budgets below T / 16 refine */
        c4.push_back(random_seq(rng, "ACDE", rng() % 300));
    check_corpus("4 letters", c4);
    for (int i = 0; i < 300; i++) /* both cases, invalid bytes, few letters so that sets collide */
        both.push_back(random_seq(rng, "AYayCw*X", 10 + rng() % 200));
    check_corpus("both cases", both);
    for (int i = 0; i < 500; i++)
        one.push_back("wywywywy");
    one.push_back("ACDEFGHIKL");
    one.push_back("yyyyyyyyy");
    check_corpus("one key repeated", one);
    std::printf("ok %ld\n", g_checks);
    return 0;
}
