/*
 * CPU check of the DEFLATE decoder and the gzip framing (csrc/kgx_inflate.h,
 * csrc/kgx_gzip.h), run by tests/test_inflate_native.py, once as built and
 * once under AddressSanitizer + UBSan.  Stand-alone, no HIP.
 *
 * argv[1] is a list of cases, one per line; one line of output per case.
 * Every input is copied into a heap block of exactly its size and every
 * output goes to a heap block of exactly the room stated, so that a read or a
 * store outside [in, in_end) or [out, out_end) is a sanitizer report.
 *
 *   raw IN OUT CAP    one raw deflate stream
 *     -> raw <reason> <bit_pos> <out_len> <in_used> <stats x 8>
 *   gz IN OUT CAP     a gzip body, every member (CAP: room for plain members' text)
 *     -> gz <reason> <member> <bit_pos> <out_len> <members> <blocked> <stats x 8>
 *        reason of the first failing member (0: none); the other members'
 *        text is still written, a failing member's slot is left as 0xA5
 *   crc IN            CRC-32 bytewise, and as 64 slices joined (the kernel's way)
 *     -> crc <bytewise hex> <joined hex>
 *   trunc IN          every proper prefix of one blocked member's deflate
 *                     data, decoded into room for ISIZE
 *     -> trunc <prefixes> <failed> <ok>
 *   pack IN OUT       many raw streams, each with its room, from one file
 *                     (run_pack), the results and outputs into OUT
 *     -> pack <streams> <ok> <failed>
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "kgx_gzip.h"

using namespace kgx;

struct Heap { /* exactly n bytes (n = 0: one byte nobody may touch is not given either) */
    uint8_t *p;
    size_t n;
    explicit Heap(size_t n_) : p(static_cast<uint8_t *>(std::malloc(n_ ? n_ : 1))), n(n_) {}
    Heap(const Heap &) = delete;
    ~Heap() { std::free(p); }
};

static bool slurp(const std::string &path, std::string &out)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        return false;
    std::stringstream ss;
    ss << in.rdbuf();
    out = ss.str();
    return true;
}

static void add(InflateStats &sum, const InflateStats &s)
{
    sum.stored_blocks += s.stored_blocks;
    sum.fixed_blocks += s.fixed_blocks;
    sum.dynamic_blocks += s.dynamic_blocks;
    sum.matches += s.matches;
    sum.max_code_len = s.max_code_len > sum.max_code_len ? s.max_code_len : sum.max_code_len;
    sum.max_distance = s.max_distance > sum.max_distance ? s.max_distance : sum.max_distance;
    sum.max_length = s.max_length > sum.max_length ? s.max_length : sum.max_length;
    sum.overlap |= s.overlap;
}

static void print_stats(const InflateStats &s)
{
    std::printf(" %u %u %u %u %u %u %u %u\n", s.stored_blocks, s.fixed_blocks, s.dynamic_blocks, s.max_code_len,
                s.max_distance, s.max_length, s.overlap, s.matches);
}

static void write_out(const std::string &path, const uint8_t *p, size_t n)
{
    std::ofstream o(path, std::ios::binary);
    o.write(reinterpret_cast<const char *>(p), (std::streamsize)n);
}

static int run_raw(const std::string &data, const std::string &out_path, size_t cap)
{
    Heap in(data.size()), out(cap);
    std::memcpy(in.p, data.data(), data.size());
    auto tables = std::make_unique<InflateTables>();
    InflateStats st;
    HostIO io;
    const InflateResult r = inflate_raw(in.p, in.p + in.n, out.p, out.p + cap, tables.get(), &st, io);
    write_out(out_path, out.p, r.out_len);
    std::printf("raw %u %llu %llu %llu", r.reason, (unsigned long long)r.bit_pos, (unsigned long long)r.out_len,
                (unsigned long long)((r.bit_pos + 7) / 8));
    print_stats(st);
    return 0;
}

static int run_gz(const std::string &data, const std::string &out_path, size_t cap)
{
    Heap in(data.size());
    std::memcpy(in.p, data.data(), data.size());
    auto tables = std::make_unique<InflateTables>();
    std::string text;
    InflateStats sum{};
    uint32_t first_reason = 0;
    uint64_t first_member = 0, first_bit = 0, members = 0, blocked = 0;
    auto failed = [&](uint32_t reason, uint64_t bit) {
        if (!first_reason) {
            first_reason = reason;
            first_member = members;
            first_bit = bit;
        }
    };
    size_t pos = 0;
    while (pos < in.n) {
        GzipHeader h;
        uint32_t reason = 0;
        const int hr = gzip_header(in.p + pos, in.n - pos, &h, &reason);
        if (hr == GZ_HDR_BAD) {
            if (!(reason == GZ_NOT_GZIP && members))
                failed(reason, 0);
            break;
        }
        if (hr == GZ_HDR_MORE) {
            failed(GZ_TRUNCATED, 0);
            break;
        }
        InflateStats st{};
        if (h.blocked) {
            GzipBlocked b;
            const int br = gzip_blocked_extent(in.p + pos, in.n - pos, h, &b);
            if (br) {
                failed(br == 1 ? (uint32_t)GZ_TRUNCATED : (uint32_t)br - 2, 0);
                break;
            }
            /* the member's data alone, in a block of its own size */
            Heap data_only(b.data_len + 8), out(b.isize);
            std::memcpy(data_only.p, in.p + pos + h.header_len, b.data_len + 8);
            std::memset(out.p, 0xA5, b.isize);
            const InflateResult r = gzip_member_inflate(data_only.p, data_only.p + b.data_len, true, out.p, b.isize,
                                                        tables.get(), &st, nullptr);
            if (r.reason) {
                failed(r.reason, r.bit_pos);
                std::memset(out.p, 0xA5, b.isize);
            }
            text.append(reinterpret_cast<const char *>(out.p), b.isize);
            pos += b.total;
            blocked++;
        } else {
            Heap out(cap);
            const uint8_t *end = nullptr;
            const InflateResult r = gzip_member_inflate(in.p + pos + h.header_len, in.p + in.n, false, out.p, cap,
                                                        tables.get(), &st, &end);
            if (r.reason) {
                failed(r.reason == INF_INPUT_END ? (uint32_t)GZ_TRUNCATED : r.reason, r.bit_pos);
                break;
            }
            text.append(reinterpret_cast<const char *>(out.p), r.out_len);
            pos = (size_t)(end - in.p);
        }
        add(sum, st);
        members++;
    }
    write_out(out_path, reinterpret_cast<const uint8_t *>(text.data()), text.size());
    std::printf("gz %u %llu %llu %llu %llu %llu", first_reason, (unsigned long long)first_member,
                (unsigned long long)first_bit, (unsigned long long)text.size(), (unsigned long long)members,
                (unsigned long long)blocked);
    print_stats(sum);
    return 0;
}

static int run_crc(const std::string &data)
{
    Heap in(data.size());
    std::memcpy(in.p, data.data(), data.size());
    const uint32_t whole = crc32_of(in.p, in.n);
    const uint32_t n = (uint32_t)in.n, slice = (n + 63u) / 64u;
    uint32_t joined = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint32_t a = lane * slice < n ? lane * slice : n, b = a + slice < n ? a + slice : n;
        const uint32_t reg = crc32_run(crc32_table(), lane == 0 ? 0xffffffffu : 0u, in.p + a, b - a);
        joined ^= crc32_mulmod(reg, crc32_xpow8(n - b));
    }
    std::printf("crc %08x %08x\n", whole, ~joined);
    return 0;
}

static int run_trunc(const std::string &data)
{
    GzipHeader h;
    GzipBlocked b;
    uint32_t reason = 0;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(data.data());
    if (gzip_header(p, data.size(), &h, &reason) != GZ_HDR_OK || !h.blocked ||
        gzip_blocked_extent(p, data.size(), h, &b) != 0) {
        std::printf("trunc not-a-blocked-member\n");
        return 0;
    }
    auto tables = std::make_unique<InflateTables>();
    unsigned failed = 0, ok = 0;
    for (uint32_t k = 0; k < b.data_len; k++) {
        Heap in(k), out(b.isize);
        std::memcpy(in.p, p + h.header_len, k);
        InflateStats st;
        HostIO io;
        const InflateResult r = inflate_raw(in.p, in.p + k, out.p, out.p + b.isize, tables.get(), &st, io);
        if (r.reason)
            failed++;
        else
            ok++;
    }
    std::printf("trunc %u %u %u\n", b.data_len, failed, ok);
    return 0;
}

/* many raw streams from one file, each a record {u32 length, u32 room, bytes};
 * OUT gets a record per stream: {u32 reason, u32 out_len, u64 bit_pos,
 * u32 stats[8], the out_len bytes}.  Input and room are heap blocks of exactly
 * their size, as for the single cases. */
static int run_pack(const std::string &data, const std::string &out_path)
{
    std::ofstream o(out_path, std::ios::binary);
    auto tables = std::make_unique<InflateTables>();
    unsigned n = 0, ok = 0, failed = 0;
    size_t at = 0;
    while (at + 8 <= data.size()) {
        uint32_t len, cap;
        std::memcpy(&len, data.data() + at, 4);
        std::memcpy(&cap, data.data() + at + 4, 4);
        at += 8;
        if (len > data.size() - at)
            break;
        Heap in(len), out(cap);
        std::memcpy(in.p, data.data() + at, len);
        at += len;
        InflateStats st;
        HostIO io;
        const InflateResult r = inflate_raw(in.p, in.p + len, out.p, out.p + cap, tables.get(), &st, io);
        if (r.out_len > cap) { /* never; and then not read back either */
            std::printf("pack stream %u: out_len %llu above its room %u\n", n, (unsigned long long)r.out_len, cap);
            return 0;
        }
        const uint32_t head[2] = {r.reason, (uint32_t)r.out_len};
        const uint64_t bit = r.bit_pos;
        const uint32_t s[8] = {st.stored_blocks, st.fixed_blocks, st.dynamic_blocks, st.max_code_len,
                               st.max_distance,  st.max_length,   st.overlap,        st.matches};
        o.write(reinterpret_cast<const char *>(head), sizeof head);
        o.write(reinterpret_cast<const char *>(&bit), sizeof bit);
        o.write(reinterpret_cast<const char *>(s), sizeof s);
        o.write(reinterpret_cast<const char *>(out.p), (std::streamsize)r.out_len);
        n++;
        if (r.reason)
            failed++;
        else
            ok++;
    }
    std::printf("pack %u %u %u\n", n, ok, failed);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: inflate_check CASES\n");
        return 2;
    }
    std::ifstream cases(argv[1]);
    std::string line;
    while (std::getline(cases, line)) {
        std::istringstream ls(line);
        std::string mode, in_path, out_path;
        size_t cap = 0;
        ls >> mode >> in_path >> out_path >> cap;
        std::string data;
        if (mode.empty())
            continue;
        if (!slurp(in_path, data)) {
            std::printf("%s cannot-read %s\n", mode.c_str(), in_path.c_str());
            continue;
        }
        if (mode == "raw")
            run_raw(data, out_path, cap);
        else if (mode == "gz")
            run_gz(data, out_path, cap);
        else if (mode == "crc")
            run_crc(data);
        else if (mode == "trunc")
            run_trunc(data);
        else if (mode == "pack")
            run_pack(data, out_path);
        else
            std::printf("%s unknown-mode\n", mode.c_str());
    }
    return 0;
}
