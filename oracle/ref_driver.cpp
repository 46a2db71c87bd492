/*
 * ref_driver.cpp -- C entry points over the parts of the reference that build
 * from their own sources with the stock toolchain:
 *
 *   kmer_encoder.cc (+ kguts.h, kmer_image.h, kmer_params.h, kmer_encoder.h)
 *   fasta_parser.cc (+ fasta_parser.h)
 *   trans_table.cc  (+ trans_table.h)
 *   kguts.h's header-only KmerOtuStats (finalize / std::sort tie order)
 *   kguts.cc        KmerGuts: the probe loop, gather_hits, process_set_of_hits,
 *                   find_best_call, format_*, insert_kmer, save_kmer_hash_table
 *   kmer_image.cc   KmerImage: mapping a data directory's kmer.table.mem_map
 *   fastq_parser.cc (+ fastq_parser.h) FastqParser
 *
 * TEST INFRASTRUCTURE ONLY.  Compiled by oracle/Makefile with
 * -Istandin -I$(REF) straight from the read-only reference tree into
 * oracle/_ref/libref.so; used to pin the oracle restatement and to record the
 * reference's answers (tests/golden/make_reference_runs.py).  kguts.cc and
 * kmer_image.cc include two boost headers but use nothing from them beyond a
 * global's type and an absent option; oracle/standin/boost/ declares those
 * two types.  This file defines the globals of global.h.  Not built:
 * dna_seq.cc (boost::split would have to be implemented, which is a
 * restatement), the asio handlers, build_signature_kmers.cc, unique_prots.cc
 * (DESIGN.md "Oracle").
 *
 * The reference prints to stdout and stderr ("mmap ...", "delete kguts ...",
 * "Error found: ..."); callers ignore that.
 */
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cmath>
#include <map>
#include <memory>
#include <sstream>

#include <boost/program_options.hpp>
#define DEFINE_GLOBALS
#include "global.h"
#include "kguts.h"
#include "kmer_encoder.h"
#include "fastq_parser.h"
#include "fasta_parser.h"
#include "trans_table.h"

extern "C" {

/* KmerEncoder::encoded_aa_kmer (kmer_encoder.h:212-225) */
unsigned long long ref_encode(const char *kmer)
{
    static KmerEncoder enc;
    return enc.encoded_aa_kmer(kmer);
}

/* KmerEncoder::decoded_kmer (kmer_encoder.h:245-255) */
void ref_decode(unsigned long long key, char *out9)
{
    static KmerEncoder enc;
    enc.decoded_kmer(key, out9);
}

/* KmerEncoder::to_amino_acid_off (kmer_encoder.h:189-191); byte 255 is left
 * uninitialised by the constructor (kmer_encoder.cc:9), callers skip it. */
int ref_residue_code(int c)
{
    static KmerEncoder enc;
    return enc.to_amino_acid_off((uint8_t)c);
}

/* KmerOtuStats::finalize (kguts.h:214-218): fill otu_map with (otu, count)
 * pairs, finalize, and return otus_by_count in out_pairs (2*n ints). */
int ref_otu_finalize(const int *otus, const int *counts, int n, int *out_pairs)
{
    KmerOtuStats s;
    for (int i = 0; i < n; i++)
        s.otu_map[otus[i]] += counts[i];
    s.finalize();
    int k = 0;
    for (auto &p : s.otus_by_count) {
        out_pairs[2 * k] = p.first;
        out_pairs[2 * k + 1] = p.second;
        k++;
    }
    return k;
}

/* FastaParser (fasta_parser.h:38-165, fasta_parser.cc:1-36): parse text, then
 * return records as "id\tseq\n" lines in a malloc'd buffer. */
char *ref_fasta_parse(const char *text, unsigned long len)
{
    std::string out;
    FastaParser parser;
    parser.set_callback([&out](const std::string &id, const std::string &seq) {
        out += id;
        out += '\t';
        out += seq;
        out += '\n';
        return 0;
    });
    parser.set_error_callback([](const std::string &, int, const std::string) { return true; });
    for (unsigned long i = 0; i < len; i++)
        parser.parse_char(text[i]);
    parser.parse_complete();
    char *buf = (char *)std::malloc(out.size() + 1);
    std::memcpy(buf, out.data(), out.size());
    buf[out.size()] = 0;
    return buf;
}

void ref_free(void *p) { std::free(p); }

/* TranslationTable::make_table(11).translate (trans_table.cc:17-84) */
char *ref_translate11(const char *dna, unsigned long len)
{
    static TranslationTable t = TranslationTable::make_table(11);
    std::string s(dna, len);
    std::string p = t.translate(s.begin(), s.end());
    char *buf = (char *)std::malloc(p.size() + 1);
    std::memcpy(buf, p.data(), p.size());
    buf[p.size()] = 0;
    return buf;
}

/* ---- KmerGuts over a KmerImage (kguts.cc, kmer_image.cc) ---- */

/* the caller's record layouts (oracle/__init__.py HIT_DTYPE, CALL_DTYPE) */
struct DrvHit {
    unsigned long long which_kmer;
    int otu_index;
    unsigned short avg_from_end;
    unsigned short reserved;
    int function_index;
    float function_wt;
    unsigned int pos;
    unsigned int seq;
};
static_assert(sizeof(DrvHit) == 32, "HIT_DTYPE is 32 bytes");
struct DrvCall {
    unsigned int start, end;
    int count;
    unsigned int function_index;
    float weighted_hits;
};
static_assert(sizeof(DrvCall) == 20, "CALL_DTYPE is 20 bytes");

struct RefKg {
    std::shared_ptr<KmerImage> image;
    KmerGuts *kg = nullptr;
    std::vector<DrvHit> hits;
    std::vector<DrvCall> calls;
    std::vector<std::pair<int, int>> otus;
};

static void copy_text(const std::string &s, char *buf, unsigned long cap)
{
    unsigned long n = s.size() < cap ? s.size() : (cap ? cap - 1 : 0);
    if (cap) {
        std::memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
}

/* KmerImage(data_dir) + KmerGuts(data_dir, image) (kmer_image.cc:15-108,
 * kguts.cc:35-58,659-679): the files close_kmers_amd.image_files writes */
void *ref_kg_open(const char *data_dir)
{
    static boost::program_options::variables_map no_options;
    g_parameters = &no_options;
    RefKg *h = new RefKg;
    h->image = std::make_shared<KmerImage>(data_dir);
    h->kg = new KmerGuts(data_dir, h->image);
    return h;
}

void ref_kg_close(void *p)
{
    RefKg *h = static_cast<RefKg *>(p);
    delete h->kg;
    h->image->detach();
    delete h;
}

/* set_parameters + process_aa_seq (kguts.cc:244-268,888-908) with calls, a hit
 * callback and OTU stats.  params4 = min_hits, max_gap, order_constraint,
 * min_weighted_hits.  seq holds no NUL.  counts3 = hits, calls, otus; the rows
 * stay in the handle until ref_kg_fetch. */
void ref_kg_process_aa(void *p, const int *params4, const char *seq, unsigned long len,
                       unsigned long long *counts3)
{
    RefKg *h = static_cast<RefKg *>(p);
    h->kg->set_parameters({{"min_hits", std::to_string(params4[0])},
                           {"max_gap", std::to_string(params4[1])},
                           {"order_constraint", std::to_string(params4[2])},
                           {"min_weighted_hits", std::to_string(params4[3])}});
    auto calls = std::make_shared<std::vector<KmerCall>>();
    auto stats = std::make_shared<KmerOtuStats>();
    h->hits.clear();
    h->calls.clear();
    h->otus.clear();
    std::vector<DrvHit> &out = h->hits;
    h->kg->process_aa_seq("s", std::string(seq, len), calls,
                          [&out](KmerGuts::hit_in_sequence_t k) {
                              DrvHit d;
                              std::memset(&d, 0, sizeof(d));
                              d.which_kmer = k.hit.which_kmer;
                              d.otu_index = k.hit.otu_index;
                              d.avg_from_end = k.hit.avg_from_end;
                              d.function_index = k.hit.function_index;
                              d.function_wt = k.hit.function_wt;
                              d.pos = k.offset;
                              out.push_back(d);
                          },
                          stats);
    for (auto &c : *calls)
        h->calls.push_back({c.start, c.end, c.count, c.function_index, c.weighted_hits});
    h->otus = stats->otus_by_count;
    counts3[0] = h->hits.size();
    counts3[1] = h->calls.size();
    counts3[2] = h->otus.size();
}

void ref_kg_fetch(void *p, void *hits, void *calls, int *otu_pairs)
{
    RefKg *h = static_cast<RefKg *>(p);
    if (hits && !h->hits.empty())
        std::memcpy(hits, h->hits.data(), h->hits.size() * sizeof(DrvHit));
    if (calls && !h->calls.empty())
        std::memcpy(calls, h->calls.data(), h->calls.size() * sizeof(DrvCall));
    if (otu_pairs)
        for (size_t i = 0; i < h->otus.size(); i++) {
            otu_pairs[2 * i] = h->otus[i].first;
            otu_pairs[2 * i + 1] = h->otus[i].second;
        }
}

/* find_best_call (kguts.cc:1008-1199).  out3 = score, weighted_score,
 * score_offset; the reference leaves score_offset untouched when there are no
 * calls, so it goes in as a marked NaN and *offset_set says whether it came
 * back changed. */
void ref_kg_find_best_call(void *p, const void *calls, unsigned long n, int *function_index,
                           char *function, unsigned long cap, float *out3, int *offset_set)
{
    RefKg *h = static_cast<RefKg *>(p);
    const DrvCall *c = static_cast<const DrvCall *>(calls);
    std::vector<KmerCall> v;
    for (unsigned long i = 0; i < n; i++)
        v.push_back(KmerCall(c[i].start, c[i].end, c[i].count, c[i].function_index, c[i].weighted_hits));
    const unsigned int mark = 0x7fc5a5a5u;
    float off;
    std::memcpy(&off, &mark, 4);
    std::string fn;
    h->kg->find_best_call(v, *function_index, fn, out3[0], out3[1], off);
    unsigned int back;
    std::memcpy(&back, &off, 4);
    *offset_set = back != mark;
    out3[2] = *offset_set ? off : 0.0f;
    copy_text(fn, function, cap);
}

/* format_call / format_hit / format_otu_stats (kguts.cc:939-973) */
void ref_kg_format_call(void *p, const void *call, char *buf, unsigned long cap)
{
    const DrvCall *c = static_cast<const DrvCall *>(call);
    copy_text(static_cast<RefKg *>(p)->kg->format_call(
                  KmerCall(c->start, c->end, c->count, c->function_index, c->weighted_hits)),
              buf, cap);
}

void ref_kg_format_hit(void *p, const void *hit, char *buf, unsigned long cap)
{
    const DrvHit *d = static_cast<const DrvHit *>(hit);
    sig_kmer_t s;
    std::memset(&s, 0, sizeof(s));
    s.which_kmer = d->which_kmer;
    s.otu_index = d->otu_index;
    s.avg_from_end = d->avg_from_end;
    s.function_index = d->function_index;
    s.function_wt = d->function_wt;
    copy_text(static_cast<RefKg *>(p)->kg->format_hit(KmerGuts::hit_in_sequence_t(s, d->pos)), buf, cap);
}

void ref_kg_format_otu_stats(void *p, const char *id, unsigned long size, const int *otu_pairs, int n,
                             char *buf, unsigned long cap)
{
    KmerOtuStats s;
    for (int i = 0; i < n; i++)
        s.otus_by_count.push_back({otu_pairs[2 * i], otu_pairs[2 * i + 1]});
    copy_text(static_cast<RefKg *>(p)->kg->format_otu_stats(id, size, s), buf, cap);
}

/* the loading constructor, insert_kmer in the given order, then
 * save_kmer_hash_table (kguts.cc:77-115,202-234).  The caller keeps
 * n < num_buckets / 2 (the reference exits otherwise).  The object is left
 * alive: its destructor frees index arrays this constructor never set. */
void ref_kg_build(long long num_buckets, const unsigned long long *keys, const int *fI, const int *oI,
                  const unsigned short *avg, const float *wt, unsigned long n, const char *out_file)
{
    KmerGuts *kg = new KmerGuts("", num_buckets);
    for (unsigned long i = 0; i < n; i++)
        kg->insert_kmer(keys[i], fI[i], oI[i], avg[i], wt[i]);
    kg->save_kmer_hash_table(out_file);
    free(kg->kmer_image_for_loading_);
    free(kg->pIseq);
    free(kg->cdata);
    free(kg->data);
    free(kg->pseq);
}

/* FastqParser (fastq_parser.h:40-172, fastq_parser.cc).  The error callback
 * returns !stop_at_error.  With call_parse_complete the text goes through
 * parse(stream), which ends with parse_complete(); without, byte by byte
 * through parse_char until it returns false.  Returns a malloc'd text:
 * "R\t<id>\t<seq>\n" per record in stream order (an id holds no tab or
 * newline), then "E\t<line>\t<id>\t<message>\n" for the first error if any. */
char *ref_fastq_parse(const char *text, unsigned long len, int stop_at_error, int call_parse_complete,
                      unsigned long *out_len)
{
    std::string out, err_line;
    FastqParser parser;
    parser.set_callback([&out](const std::string &id, const std::string &seq) {
        out += "R\t" + id + "\t" + seq + "\n";
        return 0;
    });
    parser.set_error_callback([&](const std::string &err, int line, const std::string id) {
        if (err_line.empty())
            err_line = "E\t" + std::to_string(line) + "\t" + id + "\t" + err + "\n";
        return !stop_at_error;
    });
    if (call_parse_complete) {
        std::istringstream in(std::string(text, len));
        parser.parse(in);
    } else {
        for (unsigned long i = 0; i < len; i++)
            if (!parser.parse_char(text[i]))
                break;
    }
    out += err_line;
    char *buf = (char *)std::malloc(out.size() + 1);
    std::memcpy(buf, out.data(), out.size());
    buf[out.size()] = 0;
    *out_len = out.size();
    return buf;
}

}  /* extern "C" */
