/*
 * kgx_fq_parse.h -- the FASTQ record parsers, host code only.
 *
 *   fq_parse         the fq handler's: FastqParser::parse_char (fastq_parser.h:
 *                    40-150) as FqProcessRequest drives it, which reports a
 *                    malformed byte and keeps going;
 *   fq_parse_strict  fastq_to_protein's: the same state machine under that
 *                    tool's error callback (fastq_to_protein.cc:49-53), which
 *                    returns false, so the first error ends the parse
 *                    (fastq_parser.cc:17-28) and the record in progress is
 *                    handed over as it stands (parse_complete).
 *
 * Both append to the same outputs: the current record's bases are built in
 * place at the end of `bases` (the caller sizes it: at most one byte per byte
 * parsed), a record adds its end to roff and its id to id_chars / id_off.
 * No device code and no other project header: tests/native/fq_parse_check.cpp
 * compiles this file alone.
 */
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace kgx {

enum { FQ_START, FQ_ID, FQ_DEF, FQ_DATA, FQ_PLUS_START, FQ_PLUS, FQ_QUAL };

/* every byte a letter (isalpha in the C locale: A-Z, a-z): a branch-free
 * reduction the compiler vectorises */
inline bool all_letters(const char *s, size_t n)
{
    unsigned bad = 0;
    for (size_t i = 0; i < n; i++)
        bad |= (unsigned)((unsigned char)((unsigned char)s[i] | 0x20u) - (unsigned char)'a') >= 26u;
    return bad == 0;
}

inline bool is_letter(char c) { return (unsigned char)((unsigned char)c | 0x20u) - (unsigned char)'a' < 26u; }

/* FastqParser::parse_char (fastq_parser.h:40-150), line-at-a-time, over
 * [p, end): the id runs to the first blank, sequence lines keep isalpha()
 * characters only (others are reported there and dropped), '+' and quality
 * lines are skipped; a record is emitted at the quality line's newline.  The
 * current record's residues are built in place at the end of `bases` (the
 * caller sizes it: at most one byte per byte parsed); `state` and `id` carry
 * the parser across calls. */
inline void fq_parse(const char *p, const char *end, int &state, std::string &id, char *bases, size_t &n_bases,
                     std::vector<uint64_t> &roff, std::string &id_chars, std::vector<uint64_t> &id_off)
{
    size_t nb = n_bases;
    while (p < end) {
        switch (state) {
        case FQ_START:
            if (*p++ == '@')
                state = FQ_ID;
            break;
        case FQ_ID: {
            const char *q = p;
            while (q < end && *q != ' ' && *q != '\t' && *q != '\n')
                q++;
            id.append(p, (size_t)(q - p));
            if (q < end)
                state = *q == '\n' ? FQ_DATA : FQ_DEF;
            p = q < end ? q + 1 : end;
            break;
        }
        case FQ_DEF:
        case FQ_PLUS:
        case FQ_QUAL: {
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            if (!nl) {
                p = end;
                break;
            }
            p = nl + 1;
            if (state == FQ_QUAL) { /* emit */
                id_chars += id;
                id_off.push_back(id_chars.size());
                roff.push_back(nb);
                id.clear();
                state = FQ_START;
            } else {
                state = state == FQ_DEF ? FQ_DATA : FQ_QUAL;
            }
            break;
        }
        case FQ_DATA: {
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            const char *stop = nl ? nl : end;
            const size_t L = (size_t)(stop - p);
            if (all_letters(p, L)) { /* the usual line: copied whole */
                std::memcpy(bases + nb, p, L);
                nb += L;
            } else {
                for (const char *q = p; q < stop; q++)
                    if (is_letter(*q))
                        bases[nb++] = *q;
            }
            p = stop;
            if (nl) {
                p = nl + 1;
                state = FQ_PLUS_START;
            }
            break;
        }
        case FQ_PLUS_START:
            if (*p++ == '+')
                state = FQ_PLUS;
            break;
        }
    }
    n_bases = nb;
}

/* the strict parser's state across blocks of one file */
struct FqStrict {
    int state = FQ_START;
    uint32_t line = 1;     /* 1 + newlines read (FastqParser::line_number) */
    bool stopped = false;  /* the first error was met: nothing more is read */
    uint32_t err_line = 0; /* its line (0: no error) */
    std::string err;       /* its text, as the reference words it */
    std::string err_id;    /* the id in progress there */
    std::string id;        /* the record in progress */
    void reset() { *this = FqStrict(); }
    /* the reference's report of the error (fastq_parser.h:144), without the newline */
    std::string message() const
    {
        return err_line ? "Error found: " + err + " at line " + std::to_string(err_line) + " id='" + err_id + "'"
                        : std::string();
    }
};

namespace fq_strict_detail {
inline void emit(FqStrict &s, size_t nb, std::vector<uint64_t> &roff, std::string &id_chars,
                 std::vector<uint64_t> &id_off)
{
    id_chars += s.id;
    id_off.push_back(id_chars.size());
    roff.push_back(nb);
    s.id.clear();
    s.state = FQ_START;
}
}  // namespace fq_strict_detail

/* fq_parse's framing with the tool's rule for errors: '>' or anything but
 * '@' where a record starts, a sequence byte that is no letter ('\r'
 * included), anything but '+' after the sequence line.  The first of them is
 * recorded in s, the record in progress is emitted with the id and bases it
 * has (an empty id is emitted too: the translation skips it, as the tool's
 * callback does) and nothing after it is read, in this or any later block. */
inline void fq_parse_strict(const char *p, const char *end, FqStrict &s, char *bases, size_t &n_bases,
                            std::vector<uint64_t> &roff, std::string &id_chars, std::vector<uint64_t> &id_off)
{
    size_t nb = n_bases;
    auto fail = [&](const std::string &what) {
        s.err = what;
        s.err_line = s.line;
        s.err_id = s.id;
        s.stopped = true;
        fq_strict_detail::emit(s, nb, roff, id_chars, id_off);
    };
    while (p < end && !s.stopped) {
        switch (s.state) {
        case FQ_START: {
            const char c = *p++;
            s.line += c == '\n';
            if (c == '@')
                s.state = FQ_ID;
            else
                fail(c == '>' ? "Starts with >. Is this a fasta file not a fastq file?" : "Missing @");
            break;
        }
        case FQ_ID: {
            const char *q = p;
            while (q < end && *q != ' ' && *q != '\t' && *q != '\n')
                q++;
            s.id.append(p, (size_t)(q - p));
            if (q < end) {
                s.state = *q == '\n' ? FQ_DATA : FQ_DEF;
                s.line += *q == '\n';
            }
            p = q < end ? q + 1 : end;
            break;
        }
        case FQ_DEF:
        case FQ_PLUS:
        case FQ_QUAL: {
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            if (!nl) {
                p = end;
                break;
            }
            p = nl + 1;
            s.line++;
            if (s.state == FQ_QUAL)
                fq_strict_detail::emit(s, nb, roff, id_chars, id_off);
            else
                s.state = s.state == FQ_DEF ? FQ_DATA : FQ_QUAL;
            break;
        }
        case FQ_DATA: {
            const char *nl = static_cast<const char *>(std::memchr(p, '\n', (size_t)(end - p)));
            const char *stop = nl ? nl : end;
            size_t L = (size_t)(stop - p);
            if (!all_letters(p, L)) { /* up to the first byte that is no letter */
                L = 0;
                while (is_letter(p[L]))
                    L++;
                stop = nullptr;
            }
            std::memcpy(bases + nb, p, L);
            nb += L;
            if (!stop) {
                fail(std::string("Bad data character '") + p[L] + "'");
                break;
            }
            p = stop;
            if (nl) {
                p = nl + 1;
                s.line++;
                s.state = FQ_PLUS_START;
            }
            break;
        }
        case FQ_PLUS_START: {
            const char c = *p++;
            s.line += c == '\n';
            if (c == '+')
                s.state = FQ_PLUS;
            else
                fail("Missing +");
            break;
        }
        }
    }
    n_bases = nb;
}

/* the end of the input (FastqParser::parse_complete): the record in progress
 * is emitted when it has an id -- a file without a final newline; the bases
 * of a record without one are dropped (the caller resets n_bases to the last
 * record's end).  Leaves s ready for the next file. */
inline void fq_parse_strict_finish(FqStrict &s, size_t n_bases, std::vector<uint64_t> &roff, std::string &id_chars,
                                   std::vector<uint64_t> &id_off)
{
    if (!s.stopped && !s.id.empty())
        fq_strict_detail::emit(s, n_bases, roff, id_chars, id_off);
}

}  // namespace kgx
