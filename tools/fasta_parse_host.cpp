/*
 * fasta_parse_host.cpp -- kgx::parse_fasta_body_flat (csrc/kgx_handlers.cpp:
 * the handlers' host framing of a FASTA body) behind a C interface, for
 * tools/bench_fasta_parse.py: one call parses a text on the calling thread and
 * keeps the flat batch (residues, offsets) for a kgx_process_batch that
 * follows.  BENCH INFRASTRUCTURE ONLY; built into tools/_build, linked against
 * libkgx.so.
 */
#include <chrono>
#include <cstddef>
#include <cstdint>

#include "kgx_handlers.h"

extern "C" {

/* parse text[0, n); *ms = the parse's wall clock */
void *fph_parse(const char *text, size_t n, double *ms)
{
    const auto t0 = std::chrono::steady_clock::now();
    kgx::FastaFlat *f = new kgx::FastaFlat(kgx::parse_fasta_body_flat(text, n));
    *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return f;
}

uint64_t fph_size(void *h) { return static_cast<kgx::FastaFlat *>(h)->size(); }
const char *fph_residues(void *h) { return static_cast<kgx::FastaFlat *>(h)->res.data(); }
uint64_t fph_n_residues(void *h) { return static_cast<kgx::FastaFlat *>(h)->res.size(); }
const uint64_t *fph_offsets(void *h) { return static_cast<kgx::FastaFlat *>(h)->off.data(); }
void fph_free(void *h) { delete static_cast<kgx::FastaFlat *>(h); }

}  // extern "C"
