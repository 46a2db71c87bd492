/*
 * fq_parse_check.cpp -- the FASTQ parsers of csrc/kgx_fq_parse.h on the CPU,
 * for tests/test_f2p_host.py.  Host code only.
 *
 *     fq_parse_check FILE BLOCK strict|handler
 *
 * parses FILE in blocks of BLOCK bytes, each block copied into a buffer of
 * exactly its size (so a sanitizer build sees any read past a block), and
 * prints one line per record, "R<TAB>id<TAB>bases", then for the strict parser
 * "E<TAB>line<TAB>id<TAB>report" if it met an error.
 *
 *     fq_parse_check sniff HELD BLOCK FINISHED FRESH [HELD BLOCK FINISHED FRESH ...]
 *
 * prints gzip_sniff's decision (csrc/kgx_gzip.h) for each case, one word per
 * line; HELD and BLOCK are bytes in hex ("-" for none), FINISHED and FRESH 0
 * or 1.  The bytes are copied into buffers of exactly their size.
 */
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>

#include "kgx_fq_parse.h"
#include "kgx_gzip.h"

static std::unique_ptr<char[]> from_hex(const std::string &hex, size_t *n)
{
    *n = hex == "-" ? 0 : hex.size() / 2;
    std::unique_ptr<char[]> buf(new char[*n]);
    for (size_t i = 0; i < *n; i++)
        buf[i] = (char)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
    return buf;
}

static int sniff_cases(int argc, char **argv)
{
    static const char *const names[] = {"UNKNOWN", "HELD", "TEXT", "GZIP"};
    if ((argc - 2) % 4)
        return 2;
    for (int i = 2; i < argc; i += 4) {
        size_t n_held, n;
        const auto held = from_hex(argv[i], &n_held), block = from_hex(argv[i + 1], &n);
        std::cout << names[kgx::gzip_sniff(held.get(), n_held, block.get(), n, std::atoi(argv[i + 2]) != 0,
                                           std::atoi(argv[i + 3]) != 0)]
                  << "\n";
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 2 && std::string(argv[1]) == "sniff")
        return sniff_cases(argc, argv);
    if (argc != 4) {
        std::fprintf(stderr, "usage: fq_parse_check FILE BLOCK strict|handler | sniff CASES...\n");
        return 2;
    }
    std::ifstream in(argv[1], std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const size_t block = (size_t)std::strtoull(argv[2], nullptr, 10);
    const bool strict = std::string(argv[3]) == "strict";
    if (!in.good() && !in.eof())
        return 2;
    if (!block)
        return 2;
    std::vector<char> bases(text.size() + 1);
    size_t n_bases = 0;
    std::vector<uint64_t> roff{0}, id_off{0};
    std::string id_chars, id;
    int state = kgx::FQ_START;
    kgx::FqStrict s;
    for (size_t pos = 0; pos < text.size(); pos += block) {
        const size_t n = std::min(block, text.size() - pos);
        std::unique_ptr<char[]> buf(new char[n]);
        std::memcpy(buf.get(), text.data() + pos, n);
        if (strict)
            kgx::fq_parse_strict(buf.get(), buf.get() + n, s, bases.data(), n_bases, roff, id_chars, id_off);
        else
            kgx::fq_parse(buf.get(), buf.get() + n, state, id, bases.data(), n_bases, roff, id_chars, id_off);
    }
    if (strict)
        kgx::fq_parse_strict_finish(s, n_bases, roff, id_chars, id_off);
    for (size_t r = 0; r + 1 < roff.size(); r++) {
        std::cout << "R\t" << id_chars.substr(id_off[r], id_off[r + 1] - id_off[r]) << "\t";
        std::cout.write(bases.data() + roff[r], (std::streamsize)(roff[r + 1] - roff[r]));
        std::cout << "\n";
    }
    if (strict && s.err_line)
        std::cout << "E\t" << s.err_line << "\t" << s.err_id << "\t" << s.message() << "\n";
    return 0;
}
