/*
 * kgx_f2p.cpp -- fastq_to_protein as a streaming handle (include/kgx.h
 * kgx_f2p_*): FASTQ in blocks, text or gzip (the front end
 * it shares with the fq handler of kguts_fq.cpp: GzipBodyReader, kgx_gzip.h)
 * -> the strict parser (kgx_fq_parse.h) -> parts of at most part_bytes of text -> kgx_fq_proteins on
 * the handle's context -> the part's text copied into pinned host memory.
 * One context and one part at a time: a part's download does not overlap the
 * next part's kernels.
 *
 * With the context's option "fq_parse_device" at 1 when a file starts, the
 * strict parser runs on the device instead: a part's text -- the tail the
 * last part did not consume, then new bytes (kgx_fq_parts.h) -- is uploaded
 * and framed by kgx_fq_parse, and kgx_fq_proteins_device reads the reads where
 * that left them.
 */
#include <chrono>

#include "kgx_fq_parse.h"
#include "kgx_fq_parts.h"
#include "kgx_gzip.h"
#include "kgx_rt.h"

using namespace kgx;

struct kgx_f2p {
    kgx_ctx *ctx = nullptr;
    uint64_t part_bytes = 0;
    GzipBodyReader body; /* the file being read, text or gzip: decided by its first bytes */
    /* the part being parsed */
    FqStrict ps;
    PinnedVec<char> bases;
    size_t n_bases = 0;
    std::vector<uint64_t> roff{0}, id_off{0};
    std::string id_chars;
    uint64_t part_taken = 0; /* FASTQ bytes parsed into it */
    /* "fq_parse_device" 1: the part's text, carried tail first */
    bool device_parse = false;
    FqParts parts;
    PinnedVec<char> part;
    /* this call's text */
    PinnedVec<char> out;
    size_t out_len = 0;
    std::vector<hipEvent_t> ev; /* download: start, end */
    kgx_f2p_stats st{};
    std::string err_text;
    bool ended = true; /* the last call finished a file: the next one starts the stats anew */
};

namespace {

/* a part's records, on the device, appended to the call's output; the
 * part's clocks and counts into the stats */
int take_text(kgx_f2p *h, const kgx_fq_text &t, uint32_t n)
{
    hipStream_t s = h->ctx->stream;
    if (t.n_bytes) {
        HIP_TRY(h->out.resize(h->out_len + t.n_bytes));
        HIP_TRY(hipEventRecord(h->ev[0], s));
        HIP_TRY(hipMemcpyAsync(h->out.data() + h->out_len, t.text, t.n_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(h->ev[1], s));
        HIP_TRY(host_wait(s));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
        h->st.download_ms += ms;
        h->out_len += t.n_bytes;
    }
    const float *ms = h->ctx->ft_ms;
    h->st.upload_ms += ms[0];
    h->st.index_ms += ms[1];
    h->st.sizes_ms += ms[2];
    h->st.write_ms += ms[3];
    h->st.reads += n;
    h->st.fragments += t.n_fragments;
    h->st.text_bytes += t.n_bytes;
    h->st.parts++;
    return KGX_OK;
}

/* the complete reads of the part through the device, their text appended to
 * the call's output; the record in progress moves to the front */
int flush_part(kgx_f2p *h)
{
    const uint32_t n = (uint32_t)(h->roff.size() - 1);
    if (n) {
        for (uint32_t r = 0; r < n; r++)
            h->st.reads_no_id += h->id_off[r + 1] == h->id_off[r];
        kgx_fq_text t;
        if (int rc = fq_proteins(h->ctx, h->bases.data(), h->roff.data(), h->id_chars.data(), h->id_off.data(), n, &t))
            return rc;
        if (int rc = take_text(h, t, n))
            return rc;
    }
    const size_t done = (size_t)h->roff.back();
    if (h->n_bases > done)
        std::memmove(h->bases.data(), h->bases.data() + done, h->n_bases - done);
    h->n_bases -= done;
    h->roff.assign(1, 0);
    h->id_off.assign(1, 0);
    h->id_chars.clear();
    h->part_taken = 0;
    return KGX_OK;
}

int process_text(kgx_f2p *h, const char *text, size_t n, bool finished)
{
    size_t pos = 0;
    while (pos < n && !h->ps.stopped) {
        const size_t take = (size_t)std::min<uint64_t>(n - pos, h->part_bytes - h->part_taken);
        HIP_TRY(h->bases.resize(h->n_bases + take + 16));
        const auto t0 = std::chrono::steady_clock::now();
        fq_parse_strict(text + pos, text + pos + take, h->ps, h->bases.data(), h->n_bases, h->roff, h->id_chars,
                        h->id_off);
        h->st.parse_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        pos += take;
        h->part_taken += take;
        if (h->part_taken >= h->part_bytes || h->ps.stopped)
            if (int rc = flush_part(h))
                return rc;
    }
    if (finished) {
        /* the bases of a record in progress without an id go with it */
        if (h->ps.stopped || h->ps.id.empty())
            h->n_bases = (size_t)h->roff.back();
        fq_parse_strict_finish(h->ps, h->n_bases, h->roff, h->id_chars, h->id_off);
        if (int rc = flush_part(h))
            return rc;
    }
    if (h->ps.err_line && !h->st.error_line) {
        h->st.error_line = h->ps.err_line;
        h->err_text = h->ps.message();
    }
    return KGX_OK;
}

/* the part buffer through the device parser and the translation; `last`: the
 * file ends with it.  What the parse did not consume moves to the front.  An
 * error is recorded in h->ps as the host parser records it: the text by its
 * code, the line from the newlines of the parts before, the id of the last
 * read (the record in progress, which a strict parse hands over) */
int run_part_device(kgx_f2p *h, bool last)
{
    static const char *const what[] = {"", "Starts with >. Is this a fasta file not a fastq file?", "Missing @",
                                       "Bad data character '", "Missing +"};
    kgx_fq_reads r;
    if (int rc = kgx_fq_parse(h->ctx, h->part.data(), h->parts.have, KGX_FQ_STRICT | (last ? KGX_FQ_FINISHED : 0u), &r))
        return rc;
    h->st.parse_ms += r.parse_ms;
    h->st.upload_ms += r.upload_ms;
    if (r.n_reads) {
        kgx_fq_text t;
        if (int rc = fq_proteins_device(h->ctx, &r, &t))
            return rc;
        h->st.reads_no_id += r.n_reads_no_id;
        if (int rc = take_text(h, t, r.n_reads))
            return rc;
    }
    if (r.error) {
        uint64_t io[2] = {0, 0};
        std::string id;
        if (r.n_reads) {
            HIP_TRY(hipMemcpy(io, r.id_offsets + (r.n_reads - 1), sizeof io, hipMemcpyDeviceToHost));
            id.resize((size_t)(io[1] - io[0]));
            if (!id.empty())
                HIP_TRY(hipMemcpy(&id[0], r.ids + io[0], id.size(), hipMemcpyDeviceToHost));
        }
        h->ps.err = what[r.error < 5 ? r.error : 0];
        if (r.error == 3) {
            h->ps.err += (char)r.error_byte;
            h->ps.err += '\'';
        }
        h->ps.err_line = (uint32_t)h->parts.error_line(r.error_newlines);
        h->ps.err_id = id;
        h->ps.stopped = true;
    }
    const uint64_t left = h->parts.have - r.consumed;
    if (r.consumed && left)
        std::memmove(h->part.data(), h->part.data() + r.consumed, (size_t)left);
    h->parts.parsed(r.consumed, r.newlines, !last);
    return KGX_OK;
}

int process_text_device(kgx_f2p *h, const char *text, size_t n, bool finished)
{
    size_t pos = 0;
    while (!h->ps.stopped) {
        const uint64_t k = h->parts.take(n - pos);
        if (k) {
            HIP_TRY(h->part.resize((size_t)(h->parts.have + k)));
            parallel_memcpy(h->part.data() + h->parts.have, text + pos, (size_t)k);
            h->parts.took(k);
            pos += (size_t)k;
        }
        const bool ended = finished && pos == n;
        if (!h->parts.ready(ended))
            break;
        if (int rc = run_part_device(h, ended))
            return rc;
        if (ended)
            break;
    }
    if (h->ps.err_line && !h->st.error_line) {
        h->st.error_line = h->ps.err_line;
        h->err_text = h->ps.message();
    }
    return KGX_OK;
}

/* the file ends, in its last block or in an error: the next call starts one */
void end_file(kgx_f2p *h)
{
    h->body.reset();
    h->ps.reset();
    h->n_bases = 0;
    h->roff.assign(1, 0);
    h->id_off.assign(1, 0);
    h->id_chars.clear();
    h->part_taken = 0;
    h->parts.reset(h->part_bytes);
    h->ended = true;
}

/* a block of the file, text or gzip (GzipBodyReader sniffs the file's start
 * and inflates a block's complete members), through process_text */
int process_block(kgx_f2p *h, const char *block, size_t n, bool finished)
{
    if (h->ps.stopped && h->body.body() == GZ_BODY_GZIP) /* after a parse error nothing more is inflated */
        return KGX_OK;
    const char *text = nullptr;
    size_t len = 0;
    if (int rc = h->body.feed(h->ctx, block, n, finished, true, &text, &len))
        return rc;
    if (!text) /* held: too short to tell yet */
        return KGX_OK;
    if (h->body.gzip())
        h->st.gzip = 1;
    return h->device_parse ? process_text_device(h, text, len, finished) : process_text(h, text, len, finished);
}

}  // namespace

extern "C" {

int kgx_f2p_create(kgx_ctx *ctx, uint64_t part_bytes, kgx_f2p **out)
{
    if (!ctx || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = nullptr;
    HIP_TRY(hipSetDevice(ctx->img->device));
    std::unique_ptr<kgx_f2p> h(new kgx_f2p);
    h->ctx = ctx;
    h->part_bytes = part_bytes ? part_bytes : uint64_t(32) << 20;
    h->parts.reset(h->part_bytes);
    if (int rc = ensure_events(h->ev, 2, hipEventDefault))
        return rc;
    *out = h.release();
    return KGX_OK;
}

int kgx_f2p_destroy(kgx_f2p *h)
{
    if (h)
        for (hipEvent_t e : h->ev)
            (void)hipEventDestroy(e);
    delete h;
    return KGX_OK;
}

int kgx_f2p_process(kgx_f2p *h, const char *fastq, uint64_t n, int finished, const char **text, uint64_t *text_len)
{
    if (!h || (n && !fastq) || !text || !text_len)
        return fail(KGX_EINVAL, "null argument");
    *text = "";
    *text_len = 0;
    HIP_TRY(hipSetDevice(h->ctx->img->device));
    if (h->ended) {
        h->st = kgx_f2p_stats{};
        h->err_text.clear();
        h->ended = false;
        h->device_parse = h->ctx->opt.fq_parse_device != 0;
    }
    h->out.n = 0; /* the last call's text is not kept when the buffer grows */
    h->out_len = 0;
    int rc;
    try {
        rc = process_block(h, fastq ? fastq : "", (size_t)n, finished != 0);
    } catch (const std::exception &e) {
        rc = fail(KGX_ENOMEM, e.what());
    }
    if (rc || finished)
        end_file(h);
    if (rc)
        return rc;
    if (h->out_len) {
        *text = h->out.data();
        *text_len = h->out_len;
    }
    return KGX_OK;
}

int kgx_f2p_get_stats(const kgx_f2p *h, kgx_f2p_stats *out)
{
    if (!h || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = h->st;
    return KGX_OK;
}

const char *kgx_f2p_error(const kgx_f2p *h) { return h ? h->err_text.c_str() : ""; }

}  // extern "C"
