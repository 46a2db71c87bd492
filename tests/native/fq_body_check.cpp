/*
 * fq_body_check.cpp -- the parts of a request's blocks when the device frames
 * them (csrc/kgx_fq_body.h), on the CPU, for tests/test_fq_body_native.py.
 * Host code only.
 *
 *     fq_body_check SEED TEXTS
 *
 * makes TEXTS texts from SEED -- FASTQ records of many lengths, lenient rules,
 * a few of them far longer than the others -- and for each text, block size,
 * part size and limit (a small stand-in for KGX_FQ_PARSE_MAX) drives
 * FqBodyParts as FqRequest does, once over the text in blocks of bytes (a text
 * body) and once over the text cut into members, in blocks of members (a gzip
 * body).  The parser is a byte-wise model of the lenient kgx_fq_parse: the
 * records that end in the buffer and where the last of them ends.  The part
 * buffer is reallocated at exactly `have` bytes before every parse, so a
 * sanitizer build sees any read past it.  Checked:
 *
 *   - the records handed over during block b are exactly those whose last
 *     byte lies in block b, in order (one FamilyMapper per block);
 *   - no parse holds more than the limit, and more than the room only when a
 *     single member does not fit it;
 *   - the rest of a block goes to the host parser only when the record in
 *     progress is longer than the limit, and then the carried text is what
 *     follows the block's last complete record;
 *   - at the end of the request the carried text holds no complete record.
 *
 * Prints "ok <runs> parts <parts> fallbacks <fallbacks>" or the first
 * difference.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <string>
#include <vector>

#include "kgx_fq_body.h"

namespace {

constexpr uint64_t MEMBER_MAX = 300; /* the most text one member holds here: within every limit of the sweep */

/* the lenient parse, one byte at a time from the start state: ends[i] = one
 * past the newline that ends record i */
std::vector<uint64_t> record_ends(const char *p, size_t n)
{
    enum { START, ID, DEF, DATA, PLUS_START, PLUS, QUAL };
    std::vector<uint64_t> ends;
    int state = START;
    for (size_t i = 0; i < n; i++) {
        const char c = p[i];
        switch (state) {
        case START: if (c == '@') state = ID; break;
        case ID: if (c == ' ' || c == '\t') state = DEF; else if (c == '\n') state = DATA; break;
        case DEF: if (c == '\n') state = DATA; break;
        case DATA: if (c == '\n') state = PLUS_START; break;
        case PLUS_START: if (c == '+') state = PLUS; break;
        case PLUS: if (c == '\n') state = QUAL; break;
        case QUAL:
            if (c == '\n') {
                ends.push_back(i + 1);
                state = START;
            }
            break;
        }
    }
    return ends;
}

std::string make_text(std::mt19937_64 &rng, bool long_records)
{
    std::string t;
    const int n = 1 + (int)(rng() % 40);
    for (int i = 0; i < n; i++) {
        size_t len = rng() % 60;
        if (long_records && rng() % 9 == 0)
            len = 300 + rng() % 3000;
        if (rng() % 11 == 0)
            t += "\n";
        t += "@r" + std::to_string(i) + (rng() % 5 == 0 ? " words\n" : "\n");
        t += std::string(len, "ACGT"[rng() % 4]) + "\n+\n";
        t += (rng() % 7 == 0 ? "@" : "I") + std::string(len ? len - 1 : 0, 'I') + "\n";
    }
    if (rng() % 3 == 0)
        t += "@cut\nACG"; /* a record in progress at the request's end */
    return t;
}

struct Run {
    const std::string &text;
    std::vector<uint64_t> ends; /* the whole text's record ends */
    kgx::FqBodyParts bp;
    std::string buf;            /* the part buffer: carried text, then new bytes */
    uint64_t origin = 0;        /* the text position of buf[0] */
    size_t next_end = 0;        /* records handed over so far */
    uint64_t parts = 0, fallbacks = 0;
    std::string why;

    explicit Run(const std::string &t) : text(t), ends(record_ends(t.data(), t.size())) {}

    bool fail(const std::string &w)
    {
        if (why.empty())
            why = w;
        return false;
    }
    /* a parse of the buffer, by the device (within the limit) or the host:
     * the records must be the text's next ones */
    bool parse(bool host, uint64_t *consumed)
    {
        if (!host && buf.size() > bp.limit)
            return fail("a device parse beyond the limit");
        if (buf.size() != bp.have())
            return fail("have is not the buffer's size");
        std::unique_ptr<char[]> exact(new char[buf.size() ? buf.size() : 1]);
        std::memcpy(exact.get(), buf.data(), buf.size());
        const std::vector<uint64_t> got = record_ends(exact.get(), buf.size());
        for (uint64_t e : got) {
            if (next_end >= ends.size() || ends[next_end] != origin + e)
                return fail("a record that is not the text's next one");
            next_end++;
        }
        *consumed = got.empty() ? 0 : got.back();
        return true;
    }
    void carry(uint64_t consumed)
    {
        buf.erase(0, (size_t)consumed);
        origin += consumed;
    }
    /* the rest of a block through the host parser */
    bool host_rest(const char *rest, size_t n, uint64_t slack)
    {
        /* only for a record in progress longer than the limit (less `slack`:
         * a gzip body's part ends with a whole member) */
        const uint64_t rec_end = next_end < ends.size() ? ends[next_end] : text.size();
        if (rec_end - origin + slack <= bp.limit)
            return fail("the host parser for a record within the limit");
        buf.append(rest, n);
        bp.took(n);
        uint64_t consumed = 0;
        if (!parse(true, &consumed))
            return false;
        carry(consumed);
        bp.carried(buf.size());
        fallbacks++;
        return true;
    }
    /* after block [a, b): every record that ends in it, and no other */
    bool block_done(uint64_t b)
    {
        if (origin + buf.size() != b)
            return fail("the buffer does not end where the block does");
        if (next_end < ends.size() && ends[next_end] <= b)
            return fail("a record of the block was not handed over in it");
        if (next_end && ends[next_end - 1] != origin)
            return fail("the carried text does not begin behind the last record");
        return true;
    }
};

bool run_text(Run &r, uint64_t block, uint64_t part)
{
    const std::string &t = r.text;
    for (uint64_t a = 0; a < t.size(); a += block) {
        const uint64_t b = std::min<uint64_t>(a + block, t.size());
        uint64_t pos = a;
        r.bp.begin_block(b - a, part);
        while (pos < b) {
            if (r.bp.beyond_limit(b - pos)) {
                if (!r.host_rest(t.data() + pos, (size_t)(b - pos), 0))
                    return false;
                pos = b;
                break;
            }
            const uint64_t k = r.bp.take(b - pos);
            if (!k)
                return r.fail("a part that takes nothing");
            r.buf.append(t.data() + pos, (size_t)k);
            r.bp.took(k);
            pos += k;
            if (r.buf.size() > r.bp.room())
                return r.fail("a part beyond its room");
            uint64_t consumed = 0;
            if (!r.parse(false, &consumed))
                return false;
            r.carry(consumed);
            r.bp.parsed(consumed, b - pos);
            r.parts++;
        }
        if (!r.block_done(b))
            return false;
    }
    return true;
}

bool run_members(Run &r, const std::vector<uint32_t> &len, uint32_t per_block, uint64_t part)
{
    const std::string &t = r.text;
    uint64_t at = 0;
    for (size_t m0 = 0; m0 < len.size(); m0 += per_block) {
        const size_t m1 = std::min<size_t>(m0 + per_block, len.size());
        uint64_t bytes_in_block = 0;
        for (size_t m = m0; m < m1; m++)
            bytes_in_block += len[m];
        const uint64_t b = at + bytes_in_block;
        r.bp.begin_block(bytes_in_block, part);
        size_t i = m0;
        while (i < m1) {
            uint64_t bytes = 0;
            const uint64_t had = r.bp.have();
            const uint32_t k = r.bp.take_members(&len[i], (uint32_t)(m1 - i), &bytes);
            if (!k)
                return r.fail("a part without a member");
            if (r.bp.members_beyond_limit(bytes)) {
                if (!r.host_rest(t.data() + at, (size_t)(b - at), MEMBER_MAX))
                    return false;
                at = b;
                i = m1;
                break;
            }
            if (had + bytes > r.bp.room() && k != 1)
                return r.fail("members beyond the room");
            r.buf.append(t.data() + at, (size_t)bytes);
            r.bp.took(bytes);
            at += bytes;
            i += k;
            uint64_t consumed = 0;
            if (!r.parse(false, &consumed))
                return false;
            r.carry(consumed);
            r.bp.parsed(consumed, m1 - i);
            r.parts++;
        }
        if (!r.block_done(b))
            return false;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1;
    const int texts = argc > 2 ? std::atoi(argv[2]) : 20;
    std::mt19937_64 rng(seed);
    uint64_t runs = 0, parts = 0, fallbacks = 0;
    for (int ti = 0; ti < texts; ti++) {
        const std::string text = make_text(rng, ti % 2 == 1);
        for (uint64_t block : {uint64_t(1), uint64_t(7), uint64_t(100), uint64_t(1000), uint64_t(1) << 20})
            for (uint64_t part : {uint64_t(1), uint64_t(16), uint64_t(64), uint64_t(500), uint64_t(4096)})
                for (uint64_t limit : {uint64_t(512), uint64_t(1000), uint64_t(1) << 32}) {
                    if (block == 1 && part == 1 && text.size() > 4000)
                        continue; /* quadratic */
                    {
                        Run r(text);
                        r.bp.reset(part, limit);
                        if (!run_text(r, block, part) ||
                            (!record_ends(r.buf.data(), r.buf.size()).empty() && r.fail("a record left at the end"))) {
                            std::printf("text %d block %llu part %llu limit %llu: %s\n", ti, (unsigned long long)block,
                                        (unsigned long long)part, (unsigned long long)limit, r.why.c_str());
                            return 1;
                        }
                        runs++, parts += r.parts, fallbacks += r.fallbacks;
                    }
                    /* the same text as members of up to 300 bytes (within every limit), some empty */
                    std::vector<uint32_t> len;
                    for (uint64_t left = text.size(); left;) {
                        const uint32_t k = rng() % 13 == 0 ? 0 : (uint32_t)std::min<uint64_t>(left, 1 + rng() % MEMBER_MAX);
                        len.push_back(k);
                        left -= k;
                    }
                    len.push_back(0); /* the empty member at a file's end */
                    Run r(text);
                    r.bp.reset(part, limit);
                    const uint32_t per_block = block > 1000 ? (uint32_t)len.size() : (uint32_t)(1 + block % 5);
                    if (!run_members(r, len, per_block, part)) {
                        std::printf("text %d members per block %u part %llu limit %llu: %s\n", ti, per_block,
                                    (unsigned long long)part, (unsigned long long)limit, r.why.c_str());
                        return 1;
                    }
                    runs++, parts += r.parts, fallbacks += r.fallbacks;
                }
    }
    std::printf("ok %llu parts %llu fallbacks %llu\n", (unsigned long long)runs, (unsigned long long)parts,
                (unsigned long long)fallbacks);
    return 0;
}
