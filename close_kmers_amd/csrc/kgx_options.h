/*
 * kgx_options.h -- the context's tuning options (kgx_ctx_set_option), declared
 * once: the fields with their defaults, and a table of name, field, accepted
 * values and error text.  Header-only, no HIP: tests/native/options_check.cpp
 * checks the table on the CPU.  The public description of what each option
 * does stays in include/kgx.h (above kgx_ctx_set_option).
 */
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

namespace kgx {

inline bool probe_j_supported(int j) { return (j >= 1 && j <= 5) || j == 8; }

/* every field is named as its option and is an int64_t, so that the table
 * below is plain data; results never change with any of them */
struct CtxOptions {
    /* the probe */
    int64_t probe_variant = -1;  /* PROBE_AUTO (kgx_internal.h) */
    int64_t probe_j = 2;         /* PROBE_J_DEFAULT: windows per lane, read at the next plan */
    int64_t probe_lds_kb = 0;    /* LDS reserved per probe workgroup, caps its occupancy */
    int64_t probe_persist = 0;   /* line probe grid cap in workgroups per CU, waves stride over tiles */
    int64_t probe_filter = 1;    /* use the image's presence filter when it has one */
    int64_t line_index = 1;      /* 0 = probe the reference slots even when the image has a line index */
    int64_t probe_nt = 0;        /* 1 = the line probe's hit stores non-temporal */
    int64_t probe_serialize = 1; /* this context's probes wait for the image's previous probe */
    int64_t probe_stream = 0;    /* chained probes on the image's probe stream */
    /* plan and score */
    int64_t plan_fused = 0;        /* 0 = three kernels, 1 = one look-back launch, 2 = one workgroup */
    int64_t score_variant = 0;     /* 0 = hybrid, 1 = wave-parallel, 2 = lane only (kgx_internal.h) */
    int64_t score_wave_tiles = 16; /* probe tiles of windows per scorer wave */
    /* the lane scorer for calls without OTU output under order_constraint 0:
     * 0 = the general kernel, 1 = the lean one (at most 64 VGPRs beside the
     * probe), 2 = lean with its working lanes packed into whole waves (no
     * faster than 1 at C2: 0.4574 against 0.4576 ms per step, r17) */
    int64_t score_lean = 1;
    /* fq fragments (kgx_fq.hip) */
    int64_t fq_residues = 1; /* 1: kgx_fq_fragments writes residues; 0: anchors (kgx_fq_run_device) */
    int64_t fq_count = 1;    /* fq count pass: 1 = lane-per-read stop scan, 0 = wave-per-read translation */
    int64_t fq_probe_j = 1;  /* tile of the DNA probe (fragments as anchors), 64 x J windows; 0 = probe_j */
    int64_t fq_plan = 1;     /* 1: this context's fragments are planned elementwise (fq_plan_kernel); 0: launch_plan */
    int64_t fq_fused = 1;    /* anchors: count + scan + emit in one look-back pass (fq_anchor_fused_kernel); 0: four launches */
    /* kgx_microbench_random_read */
    int64_t microbench_span = 0; /* bytes of the table the random-read ceiling covers; 0 = all */
    int64_t microbench_ilp = 8;  /* independent reads in flight per lane */
    int64_t microbench_wgs = 8;  /* 256-thread workgroups per CU */
    /* host-buffer batches in chunks: chunks alternate between the context and
     * a twin over the same image, so one chunk's gather + D2H overlaps the
     * next chunk's H2D + kernels */
    int64_t host_chunks = 6;
    int64_t host_copy = 1;         /* chunk D2H: 0 = DMA (hipMemcpyAsync), 1 = device stores into mapped memory */
    int64_t host_copy_blocks = 64; /* workgroups of the store copy */
    /* compact chunk D2H (PACKED16 images): a chunk's hits cross PCIe as their
     * 16-byte table records plus the chunk's hit mask, and host threads expand
     * them into kgx_hit (position = mask bit) while the next chunk streams */
    int64_t host_hits16 = 1;
    int64_t host_threads = 12; /* expansion threads */
    /* chunk staging (pageable caller buffer -> pinned) in parts on this many
     * threads (1 = the calling thread) */
    int64_t stage_threads = 8; /* r4ag, 3.57-3.65 vs 3.71-3.90 ms per batch with 4 */
    /* streamed schedule, 1: every chunk's residues and offsets go up on a
     * stream of their own into a region of the batch's own (up_res / up_off),
     * as soon as they are staged, instead of behind the previous chunk's
     * kernels on the context's stream.  Off by default: with the runtime's 4
     * hardware queues per process the upload stream shares one with a stream
     * that waits on events, and measured no faster (r4l/r4m: 3.66-4.21 vs
     * 3.76-4.09 ms per 30M-residue batch; with 16 queues the uploads do run
     * early, 3.60-3.90 ms) */
    int64_t host_upload_stream = 0;
    int64_t host_score_variant = 1; /* streamed chunks' scorer (-1: score_variant) */
    /* streamed schedule (compact records only): device CSR offsets, bulk
     * copies sized on the device into host regions sized from the context's
     * rates (records per window seen so far, x 1.25) */
    int64_t host_stream = 1;
    int64_t host_taper = 1; /* first and last chunk half-size */
    /* (default 1): a streamed host batch whose residues already sit in pinned
     * memory (kgx_host_alloc, hipHostMalloc / hipHostRegister) goes to the
     * device by DMA straight from the caller's buffer, with no staging copy on
     * the host; a device scan flags NUL bytes (the host-side strlen cut,
     * kguts.cc:792) and such a batch reruns staged */
    int64_t pinned_input = 1;
    int64_t host_rec12 = 1;     /* streamed: 12-B records, key re-encoded on the host */
    int64_t host_h2d_first = 1; /* streamed: chunk k's D2H waits for chunk k+1's H2D */
    /* streamed: every chunk staged into its own region of h_res_all /
     * h_off_all, not into the context's h_res behind the H2D of the chunk two
     * before */
    int64_t host_stage_all = 0; /* r4ak: 3.61-3.70 vs 3.49-3.73 ms per batch, no gain */
    /* streamed: chunk copies by DMA (hipMemcpyAsync of each region whole, at
     * its host-sized room) instead of the counted device-store copy */
    int64_t host_stream_dma = 0;
    int64_t host_nt = 1;      /* expansion with streaming stores */
    int64_t counts_first = 1; /* chunk k's bulk D2H waits for chunk k+1's counts */
    int64_t host_profile = 0; /* per-chunk timing events and the last call's profile */
    /* small host batches (<= small_batch residues, 0 = off): planned on the
     * host, read by the device from the mapped staging blob, results stored
     * into mapped memory: one host wait per batch */
    int64_t small_batch = 1 << 21;  /* 2M residues: a 1-MiB request body and then some */
    int64_t small_wave = 1;         /* small batches: the wave scorer instead of the hybrid */
    int64_t small_wave_tiles = 1;   /* small batches: probe tiles per scorer wave */
    /* one-launch small batches (kgx_fused.hip): mapped window bases,
     * per-sequence result regions, counts and tokens */
    int64_t small_fused = 0;
    int64_t fused_inline = 1; /* a tiny fused batch travels in the kernel arguments */
    /* kgx_gunzip: blocked gzip members on the device (1) or on up to 16 host
     * threads (0).  0 by the rule the feature was given: the device path stays
     * the default only if host-to-host it beats 16 x zlib on one thread (ideal
     * scaling of the reference's method over a box's 16 CPUs) by more than its
     * own spread, at BGZF level 6 and level 1.  Measured, GB/s of output
     * (profiles/gunzip_bench.json): 16.9-17.4 against 16.4 at level 6, but
     * 13.1-13.4 against 14.1 at level 1.  This project's own 16 host threads
     * reach 5.8 and 5.1, so a caller that wants throughput sets 1 */
    int64_t gunzip_device = 0;
    /* kgx_f2p_process: a part's FASTQ text is framed on the device
     * (kgx_fq_parse, kgx_fq_parse.hip) instead of by the host's strict parser
     * (kgx_fq_parse.h).  The output is the same bytes.  Measured 2.4 times as
     * fast for 10M reads (274 against 656 ms, profiles/fq_parse_device_bench.json);
     * the default stays 0 until that is repeated on a second box (DESIGN.md
     * §8.12, §12) */
    int64_t fq_parse_device = 0;
    /* kgx_fq_process: a request's text is framed on the device part by part
     * (kgx_fq_parse, lenient), a gzip body's blocked members are inflated into
     * that text on the device, and the printed reads' ids come down through
     * kgx_fq_read_ids (kguts_fq.cpp).  The output is the same
     * bytes; the default stays 0 until a second box repeats the measurement */
    int64_t fq_body_device = 0;
};

struct CtxOptionRow {
    const char *name;
    int64_t CtxOptions::*field;
    int64_t lo, hi;         /* accepted range, unless ok is set */
    const char *must_be;    /* the error text after "<name> must be " */
    bool (*ok)(int64_t);    /* accepted values that are not a range */
};

inline bool microbench_ilp_ok(int64_t v) { return v == 1 || v == 2 || v == 4 || v == 8 || v == 16; }
inline bool probe_j_ok(int64_t v) { return probe_j_supported((int)v); }

#define KGX_OPT(name) #name, &CtxOptions::name
static const CtxOptionRow CTX_OPTION_TABLE[] = {
    {KGX_OPT(microbench_ilp), 0, 0, "1, 2, 4, 8 or 16", microbench_ilp_ok},
    {KGX_OPT(microbench_wgs), 1, 32, "1..32", nullptr},
    {KGX_OPT(microbench_span), 0, INT64_MAX, ">= 0", nullptr},
    {KGX_OPT(probe_filter), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(probe_variant), -1, 3, "-1, 0, 1, 2 or 3", nullptr},
    {KGX_OPT(plan_fused), 0, 2, "0, 1 or 2", nullptr},
    {KGX_OPT(probe_nt), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(line_index), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(probe_serialize), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_copy_blocks), 1, 4096, "1..4096", nullptr},
    {KGX_OPT(host_copy), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_hits16), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(stage_threads), 1, 64, "1..64", nullptr},
    {KGX_OPT(host_score_variant), -1, 2, "-1 (the context's score_variant) or 0..2", nullptr},
    {KGX_OPT(host_upload_stream), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_stream_dma), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(pinned_input), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_stage_all), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_h2d_first), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_rec12), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_nt), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_taper), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_stream), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(counts_first), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_threads), 1, 64, "1..64", nullptr},
    {KGX_OPT(small_batch), 0, 1 << 24, "0..16777216 residues", nullptr},
    {KGX_OPT(probe_stream), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(probe_persist), 0, 32, "0..32 workgroups per CU", nullptr},
    {KGX_OPT(small_wave), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_profile), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(host_chunks), 1, 64, "1..64", nullptr},
    {KGX_OPT(fq_count), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(fq_residues), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(score_variant), 0, 2, "0, 1 or 2", nullptr},
    {KGX_OPT(probe_lds_kb), 0, 160, "0..160", nullptr},
    {KGX_OPT(fused_inline), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(small_fused), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(small_wave_tiles), 1, 256, "1..256", nullptr},
    {KGX_OPT(score_wave_tiles), 1, 256, "1..256", nullptr},
    {KGX_OPT(fq_fused), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(fq_plan), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(fq_probe_j), 0, 4, "0 (= probe_j), 1, 2, 3 or 4", nullptr},
    {KGX_OPT(probe_j), 0, 0, "1, 2, 3, 4, 5 or 8", probe_j_ok},
};
constexpr size_t CTX_OPTION_COUNT = sizeof(CTX_OPTION_TABLE) / sizeof(CTX_OPTION_TABLE[0]);
/* options declared since, of whatever subsystem: the table above is the one
 * that tests/native/options_check.cpp holds against its own record name by
 * name (score_lean's values and text: tests/test_gpu_score_lean.py) */
static const CtxOptionRow CTX_OPTION_TABLE_LATER[] = {
    {KGX_OPT(gunzip_device), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(score_lean), 0, 2, "0, 1 or 2", nullptr},
    {KGX_OPT(fq_parse_device), 0, 1, "0 or 1", nullptr},
    {KGX_OPT(fq_body_device), 0, 1, "0 or 1", nullptr},
};
#undef KGX_OPT

inline const CtxOptionRow *ctx_option_find(const char *name)
{
    for (const CtxOptionRow &r : CTX_OPTION_TABLE)
        if (!std::strcmp(r.name, name))
            return &r;
    for (const CtxOptionRow &r : CTX_OPTION_TABLE_LATER)
        if (!std::strcmp(r.name, name))
            return &r;
    return nullptr;
}

/* 0 and o.<name> = value, or -1 and *err = the text for kgx_last_error() (o unchanged) */
inline int ctx_option_set(CtxOptions &o, const char *name, int64_t value, std::string *err)
{
    const CtxOptionRow *r = ctx_option_find(name);
    if (!r) {
        *err = std::string("unknown option ") + name;
        return -1;
    }
    if (r->ok ? !r->ok(value) : (value < r->lo || value > r->hi)) {
        *err = std::string(name) + " must be " + r->must_be;
        return -1;
    }
    o.*(r->field) = value;
    return 0;
}

inline bool ctx_option_get(const CtxOptions &o, const char *name, int64_t *value)
{
    const CtxOptionRow *r = ctx_option_find(name);
    if (r)
        *value = o.*(r->field);
    return r != nullptr;
}

}  // namespace kgx
