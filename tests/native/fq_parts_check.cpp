/*
 * fq_parts_check.cpp -- the part and tail arithmetic of csrc/kgx_fq_parts.h on
 * the CPU, for tests/test_fq_parts_native.py.  Host code only.
 *
 *     fq_parts_check SEED TEXTS
 *
 * makes TEXTS FASTQ texts from SEED (well-formed records of many lengths, some
 * texts with one offending byte, some cut short of their end), and for each
 * text, each block size and each part_bytes of the sweep drives FqParts as
 * kgx_f2p_process does: blocks in, parts out to a byte-wise model of
 * kgx_fq_parse (strict, FINISHED on the file's last part), tail carried.  The
 * part buffer is reallocated at exactly `have` bytes before every parse, so a
 * sanitizer build sees any read past it.  The records, the error's text, line
 * and id must be the whole text's under the same model in one call; no part
 * may run twice unchanged, and a part never holds more than its room.  Prints
 * "ok <runs>" or the first difference.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "kgx_fq_parts.h"

namespace {

using Record = std::pair<std::string, std::string>;

struct Parsed {
    std::vector<Record> reads;
    uint64_t consumed = 0, newlines = 0;
    uint32_t error = 0;
    unsigned char error_byte = 0;
    uint64_t error_newlines = 0;
};

bool letter(unsigned char c) { return (unsigned char)((c | 0x20u) - 'a') < 26u; }

/* kgx_fq_parse with KGX_FQ_STRICT, one byte at a time (include/kgx.h) */
Parsed model(const char *p, size_t n, bool finished)
{
    enum { START, ID, DEF, DATA, PLUS_START, PLUS, QUAL };
    Parsed out;
    int state = START;
    std::string id, seq;
    uint64_t nl = 0;
    for (size_t i = 0; i < n; i++) {
        const unsigned char c = (unsigned char)p[i];
        nl += c == '\n';
        uint32_t err = 0;
        switch (state) {
        case START: if (c == '@') state = ID; else err = c == '>' ? 1 : 2; break;
        case ID: if (c == ' ' || c == '\t') state = DEF; else if (c == '\n') state = DATA; else id += (char)c; break;
        case DEF: if (c == '\n') state = DATA; break;
        case DATA: if (c == '\n') state = PLUS_START; else if (letter(c)) seq += (char)c; else err = 3; break;
        case PLUS_START: if (c == '+') state = PLUS; else err = 4; break;
        case PLUS: if (c == '\n') state = QUAL; break;
        case QUAL:
            if (c == '\n') {
                out.reads.emplace_back(id, seq);
                id.clear();
                seq.clear();
                state = START;
                out.consumed = i + 1;
                out.newlines = nl;
            }
            break;
        }
        if (err) { /* the record in progress as it stands; nothing more is read */
            out.reads.emplace_back(id, seq);
            out.error = err;
            out.error_byte = c;
            out.error_newlines = nl;
            out.consumed = n;
            for (size_t j = i + 1; j < n; j++)
                nl += p[j] == '\n';
            out.newlines = nl;
            return out;
        }
    }
    if (finished) {
        if (!id.empty())
            out.reads.emplace_back(id, seq);
        out.consumed = n;
        out.newlines = nl;
    }
    return out;
}

struct Outcome {
    std::vector<Record> reads;
    uint32_t error = 0;
    unsigned char error_byte = 0;
    uint64_t error_line = 0;
    std::string error_id;
    uint64_t runs = 0;
};

int fail(const char *what, const std::string &text, size_t block, uint64_t part_bytes)
{
    std::printf("FAIL %s: text of %zu bytes, block %zu, part_bytes %llu\n", what, text.size(), block,
                (unsigned long long)part_bytes);
    return 1;
}

/* the handle's loop (kgx_f2p.cpp process_text_device) over the text in blocks */
int stream(const std::string &text, size_t block, uint64_t part_bytes, Outcome &o)
{
    kgx::FqParts parts;
    parts.reset(part_bytes);
    std::string buf; /* the part: buf.size() == parts.have */
    bool stopped = false;
    uint64_t last_have = UINT64_MAX;
    bool last_unconsumed = false;
    size_t at = 0;
    do {
        const size_t n = std::min(block, text.size() - at);
        const bool finished = at + n == text.size();
        size_t pos = 0;
        while (!stopped) {
            const uint64_t k = parts.take(n - pos);
            if (k > n - pos)
                return fail("take beyond the block", text, block, part_bytes);
            buf.append(text, at + pos, (size_t)k);
            parts.took(k);
            pos += (size_t)k;
            if (parts.have != buf.size() || (k && parts.have > parts.room))
                return fail("have", text, block, part_bytes);
            const bool ended = finished && pos == n;
            if (!parts.ready(ended))
                break;
            if (last_unconsumed && parts.have == last_have)
                return fail("a part ran again unchanged", text, block, part_bytes);
            /* the parse sees exactly `have` bytes */
            std::unique_ptr<char[]> exact(new char[buf.size()]);
            std::memcpy(exact.get(), buf.data(), buf.size());
            const Parsed r = model(exact.get(), buf.size(), ended);
            o.runs++;
            o.reads.insert(o.reads.end(), r.reads.begin(), r.reads.end());
            if (r.error) {
                o.error = r.error;
                o.error_byte = r.error_byte;
                o.error_line = parts.error_line(r.error_newlines);
                o.error_id = r.reads.back().first;
                stopped = true;
            }
            if (r.consumed > buf.size())
                return fail("consumed", text, block, part_bytes);
            last_have = parts.have;
            last_unconsumed = r.consumed == 0;
            buf.erase(0, (size_t)r.consumed);
            parts.parsed(r.consumed, r.newlines, !ended);
            if (ended)
                break;
        }
        if (!stopped && pos != n)
            return fail("a block's bytes left behind", text, block, part_bytes);
        at += n;
    } while (at < text.size());
    if (!stopped && parts.have)
        return fail("bytes left at the end of the file", text, block, part_bytes);
    return 0;
}

std::string make_text(std::mt19937 &rng, int kind)
{
    static const char acgt[] = "ACGTacgtNn";
    std::string t;
    const int n_rec = 1 + (int)(rng() % 40);
    const int bad = kind % 4 == 1 ? (int)(rng() % n_rec) : -1;
    for (int r = 0; r < n_rec; r++) {
        const size_t L = rng() % 5 == 0 ? rng() % 700 : rng() % 90;
        std::string id = rng() % 11 == 0 ? "" : "r" + std::to_string(r) + std::string(rng() % 6, 'x');
        std::string seq(L, 'A');
        for (char &c : seq)
            c = acgt[rng() % 10];
        if (r == bad) {
            switch (rng() % 4) {
            case 0: seq.insert(seq.size() / 2, 1, "-*\r5"[rng() % 4]); break;
            case 1: t += rng() % 2 ? ">" : "\n"; break;
            case 2: t += "@" + id + "\n" + seq + "\nI\n" + std::string(L, 'I') + "\n"; continue;
            default: id = "";
            }
        }
        t += "@" + id + (rng() % 3 == 0 ? " a definition line @+>" : "") + "\n" + seq + "\n+" +
             (rng() % 4 == 0 ? id : "") + "\n" + std::string(L, rng() % 7 == 0 ? '@' : 'I') + "\n";
    }
    if (kind % 4 == 2 && !t.empty()) /* cut short: no final newline, or somewhere in the last record */
        t.resize(t.size() - 1 - (rng() % 3 ? 0 : rng() % std::min<size_t>(t.size(), 60)));
    return t;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 3) {
        std::fprintf(stderr, "usage: fq_parts_check SEED TEXTS\n");
        return 2;
    }
    std::mt19937 rng((uint32_t)std::atol(argv[1]));
    const int texts = std::atoi(argv[2]);
    static const size_t blocks[] = {1, 7, 64, 1000, 1u << 20};
    static const uint64_t part_sizes[] = {1, 16, 64, 100, 256, 4096, 65536};
    uint64_t runs = 0, errors = 0;
    for (int i = 0; i < texts; i++) {
        const std::string text = i == 0 ? std::string() : make_text(rng, i);
        const Parsed whole = model(text.data(), text.size(), true);
        for (size_t block : blocks)
            for (uint64_t pb : part_sizes) {
                Outcome o;
                if (stream(text, block, pb, o))
                    return 1;
                runs += o.runs;
                if (o.reads != whole.reads)
                    return fail("records", text, block, pb);
                if (o.error != whole.error || o.error_byte != whole.error_byte)
                    return fail("error", text, block, pb);
                if (whole.error) {
                    errors++;
                    if (o.error_line != 1 + whole.error_newlines)
                        return fail("error line", text, block, pb);
                    if (o.error_id != whole.reads.back().first)
                        return fail("error id", text, block, pb);
                }
            }
    }
    std::printf("ok %llu runs, %llu with an error\n", (unsigned long long)runs, (unsigned long long)errors);
    return 0;
}
