/*
 * CPU check of the context's option table (kgx_options.h), run by
 * tests/test_options_native.py.  Prints "ok" or the first violation.
 *
 * ROWS below is the record of what kgx_ctx_set_option accepted, defaulted to
 * and answered when each option was its own block of code with its own field
 * in kgx_ctx; it is written out by hand and is not derived from the table it
 * checks.  Properties:
 *  1. the table holds exactly these 43 names, none twice;
 *  2. on a fresh CtxOptions every option reads back its default;
 *  3. the lowest and highest accepted value (or each member of the accepted
 *     set) is taken and read back;
 *  4. lowest - 1 and highest + 1 (or near misses of the set) are refused with
 *     exactly the recorded text, and the value stays;
 *  5. an unknown name is refused with "unknown option <name>".
 */
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "kgx_options.h"

struct Row {
    const char *name;
    int64_t def;
    int64_t lo, hi;              /* accepted range, when accepted is empty */
    std::vector<int64_t> accepted; /* accepted set */
    std::vector<int64_t> refused;  /* near misses of the set */
    const char *error;
};

static const std::vector<Row> ROWS = {
    {"microbench_ilp", 8, 0, 0, {1, 2, 4, 8, 16}, {0, 3, 32}, "microbench_ilp must be 1, 2, 4, 8 or 16"},
    {"microbench_wgs", 8, 1, 32, {}, {}, "microbench_wgs must be 1..32"},
    {"microbench_span", 0, 0, INT64_MAX, {}, {}, "microbench_span must be >= 0"},
    {"probe_filter", 1, 0, 1, {}, {}, "probe_filter must be 0 or 1"},
    {"probe_variant", -1, -1, 3, {}, {}, "probe_variant must be -1, 0, 1, 2 or 3"},
    {"plan_fused", 0, 0, 2, {}, {}, "plan_fused must be 0, 1 or 2"},
    {"probe_nt", 0, 0, 1, {}, {}, "probe_nt must be 0 or 1"},
    {"line_index", 1, 0, 1, {}, {}, "line_index must be 0 or 1"},
    {"probe_serialize", 1, 0, 1, {}, {}, "probe_serialize must be 0 or 1"},
    {"host_copy_blocks", 64, 1, 4096, {}, {}, "host_copy_blocks must be 1..4096"},
    {"host_copy", 1, 0, 1, {}, {}, "host_copy must be 0 or 1"},
    {"host_hits16", 1, 0, 1, {}, {}, "host_hits16 must be 0 or 1"},
    {"stage_threads", 8, 1, 64, {}, {}, "stage_threads must be 1..64"},
    {"host_score_variant", 1, -1, 2, {}, {},
     "host_score_variant must be -1 (the context's score_variant) or 0..2"},
    {"host_upload_stream", 0, 0, 1, {}, {}, "host_upload_stream must be 0 or 1"},
    {"host_stream_dma", 0, 0, 1, {}, {}, "host_stream_dma must be 0 or 1"},
    {"pinned_input", 1, 0, 1, {}, {}, "pinned_input must be 0 or 1"},
    {"host_stage_all", 0, 0, 1, {}, {}, "host_stage_all must be 0 or 1"},
    {"host_h2d_first", 1, 0, 1, {}, {}, "host_h2d_first must be 0 or 1"},
    {"host_rec12", 1, 0, 1, {}, {}, "host_rec12 must be 0 or 1"},
    {"host_nt", 1, 0, 1, {}, {}, "host_nt must be 0 or 1"},
    {"host_taper", 1, 0, 1, {}, {}, "host_taper must be 0 or 1"},
    {"host_stream", 1, 0, 1, {}, {}, "host_stream must be 0 or 1"},
    {"counts_first", 1, 0, 1, {}, {}, "counts_first must be 0 or 1"},
    {"host_threads", 12, 1, 64, {}, {}, "host_threads must be 1..64"},
    {"small_batch", 2097152, 0, 16777216, {}, {}, "small_batch must be 0..16777216 residues"},
    {"probe_stream", 0, 0, 1, {}, {}, "probe_stream must be 0 or 1"},
    {"probe_persist", 0, 0, 32, {}, {}, "probe_persist must be 0..32 workgroups per CU"},
    {"small_wave", 1, 0, 1, {}, {}, "small_wave must be 0 or 1"},
    {"host_profile", 0, 0, 1, {}, {}, "host_profile must be 0 or 1"},
    {"host_chunks", 6, 1, 64, {}, {}, "host_chunks must be 1..64"},
    {"fq_count", 1, 0, 1, {}, {}, "fq_count must be 0 or 1"},
    {"fq_residues", 1, 0, 1, {}, {}, "fq_residues must be 0 or 1"},
    {"score_variant", 0, 0, 2, {}, {}, "score_variant must be 0, 1 or 2"},
    {"probe_lds_kb", 0, 0, 160, {}, {}, "probe_lds_kb must be 0..160"},
    {"fused_inline", 1, 0, 1, {}, {}, "fused_inline must be 0 or 1"},
    {"small_fused", 0, 0, 1, {}, {}, "small_fused must be 0 or 1"},
    {"small_wave_tiles", 1, 1, 256, {}, {}, "small_wave_tiles must be 1..256"},
    {"score_wave_tiles", 16, 1, 256, {}, {}, "score_wave_tiles must be 1..256"},
    {"fq_fused", 1, 0, 1, {}, {}, "fq_fused must be 0 or 1"},
    {"fq_plan", 1, 0, 1, {}, {}, "fq_plan must be 0 or 1"},
    {"fq_probe_j", 1, 0, 4, {}, {}, "fq_probe_j must be 0 (= probe_j), 1, 2, 3 or 4"},
    {"probe_j", 2, 0, 0, {1, 2, 3, 4, 5, 8}, {0, 6, 7, 9}, "probe_j must be 1, 2, 3, 4, 5 or 8"},
};

static int bad(const char *what, const char *name, long long v)
{
    std::printf("FAIL %s (%s, %lld)\n", what, name, v);
    return 1;
}

int main()
{
    if (ROWS.size() != 43)
        return bad("the record does not hold 43 rows", "", (long long)ROWS.size());
    /* 1. the same names, each once */
    std::set<std::string> want, got;
    for (const Row &r : ROWS)
        want.insert(r.name);
    for (const kgx::CtxOptionRow &t : kgx::CTX_OPTION_TABLE)
        if (!got.insert(t.name).second)
            return bad("option twice in the table", t.name, 0);
    if (kgx::CTX_OPTION_COUNT != ROWS.size() || got != want) {
        for (const std::string &n : got)
            if (!want.count(n))
                return bad("option in the table, not in the record", n.c_str(), 0);
        for (const std::string &n : want)
            if (!got.count(n))
                return bad("option in the record, not in the table", n.c_str(), 0);
        return bad("table size", "", (long long)kgx::CTX_OPTION_COUNT);
    }
    for (const Row &r : ROWS) {
        std::vector<int64_t> yes = r.accepted, no = r.refused;
        if (yes.empty()) {
            yes = {r.lo, r.hi};
            no.push_back(r.lo - 1);
            if (r.hi != INT64_MAX)
                no.push_back(r.hi + 1);
        }
        for (int64_t v : yes) {
            kgx::CtxOptions o; /* fresh */
            int64_t x = INT64_MIN;
            std::string err;
            /* 2. the default */
            if (!kgx::ctx_option_get(o, r.name, &x) || x != r.def)
                return bad("default", r.name, (long long)x);
            /* 3. accepted and read back */
            if (kgx::ctx_option_set(o, r.name, v, &err) != 0 || !err.empty())
                return bad("accepted value refused", r.name, (long long)v);
            if (!kgx::ctx_option_get(o, r.name, &x) || x != v)
                return bad("value not read back", r.name, (long long)v);
            /* no other option moved */
            for (const Row &q : ROWS)
                if (&q != &r && (!kgx::ctx_option_get(o, q.name, &x) || x != q.def))
                    return bad("another option changed", q.name, (long long)x);
        }
        /* 4. refused with the recorded text, value unchanged */
        for (int64_t v : no) {
            kgx::CtxOptions o;
            int64_t x = INT64_MIN;
            std::string err;
            if (kgx::ctx_option_set(o, r.name, v, &err) == 0)
                return bad("value outside the accepted ones taken", r.name, (long long)v);
            if (err != r.error) {
                std::printf("FAIL error text for %s = %lld: \"%s\", recorded \"%s\"\n", r.name, (long long)v,
                            err.c_str(), r.error);
                return 1;
            }
            if (!kgx::ctx_option_get(o, r.name, &x) || x != r.def)
                return bad("refused value changed the option", r.name, (long long)x);
        }
    }
    /* 5. unknown names */
    for (const char *n : {"no_such_option", "", "use_line_index", "host_stream_chunks", "probe_j "}) {
        kgx::CtxOptions o;
        int64_t x = 0;
        std::string err;
        if (kgx::ctx_option_set(o, n, 1, &err) == 0 || err != std::string("unknown option ") + n)
            return bad("unknown option not refused as such", n, 0);
        if (kgx::ctx_option_get(o, n, &x))
            return bad("unknown option read", n, 0);
    }
    std::printf("ok\n");
    return 0;
}
