/*
 * kgx_line_index.hip -- what is made of an image's resident table: the
 * PACKED16 layout conversion, the presence filter, and the line index
 * (kgx_line_home.h) with its build, mark and statistics kernels and its
 * C ABI entry points (kgx_image_set_line_index, kgx_image_line_*).
 */
#include "kgx_device.h"
#include "kgx_rt.h"

namespace kgx {

/* ------------------------------------------------------------------------ */
/* resident layout conversion                                                */
/* ------------------------------------------------------------------------ */

__global__ __launch_bounds__(256) void pack_kernel(const kgx_sig_kmer *__restrict__ table,
                                                   packed_bucket *__restrict__ packed, uint64_t n,
                                                   uint32_t *not_packable)
{
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const kgx_sig_kmer e = table[i];
        bad |= !packable(e);
        packed[i] = pack_bucket(e);
    }
    if (__any(bad) && lane_id() == 0)
        atomicOr(not_packable, 1u);
}

__global__ __launch_bounds__(256) void unpack_kernel(const packed_bucket *__restrict__ packed,
                                                     kgx_sig_kmer *__restrict__ out, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = unpack_bucket(packed[i]);
}

__global__ __launch_bounds__(256) void filter_build_kernel(const void *__restrict__ table, int layout, uint64_t n,
                                                           uint64_t *__restrict__ filter, uint32_t log2_words)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = layout == KGX_LAYOUT_PACKED16
                                 ? static_cast<const packed_bucket *>(table)[i].lo & PACK_KEY_MASK
                                 : static_cast<const kgx_sig_kmer *>(table)[i].which_kmer;
        if (key > MAX_ENCODED)
            continue;
        const uint64_t h = filter_hash(key);
        atomicOr(reinterpret_cast<unsigned long long *>(filter + filter_word(h, log2_words)),
                 (unsigned long long)filter_bits(h));
    }
}

hipError_t launch_filter_build(const void *table, int layout, uint64_t num_sigs, uint64_t *filter,
                               uint32_t log2_words, hipStream_t stream)
{
    hipLaunchKernelGGL(filter_build_kernel, dim3(8192), dim3(256), 0, stream, table, layout, num_sigs, filter,
                       log2_words);
    return hipGetLastError();
}

/* stored keys of a PACKED16 table (grid-stride blocks, one atomic each) */
__global__ __launch_bounds__(256) void count_keys_kernel(const packed_bucket *__restrict__ t, uint64_t n,
                                                         unsigned long long *count)
{
    uint64_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        c += (t[i].lo & PACK_KEY_MASK) <= MAX_ENCODED;
    for (int o = 32; o > 0; o >>= 1)
        c += __shfl_xor(c, o);
    if (lane_id() == 0 && c)
        atomicAdd(count, (unsigned long long)c);
}

/* The line index (kgx_image_set_line_index): every bucket b of the reference
 * table whose key the reference's probe of that key reaches first --
 * lookup_hash_entry (kguts.cc:585-602) walks from key mod num_sigs and stops at
 * the key or at a stop bucket, so a duplicate further on or an entry behind a
 * stop is never found -- is inserted into the line table by linear probing
 * from the start of the key's home line (line_home, kgx_line_home.h), 4
 * buckets a line, by a 64-bit CAS on the record's first word.  A probe of the
 * line table from that home finds exactly the records the reference finds, so
 * results are unchanged while nearly every chain ends in its first 64-B line.
 * `home` is the index's home word and line_magic the magic of what its homes
 * are taken modulo (home_magic_lines).  Twins (the minimizer home only,
 * kgx_line_home.h): the record is inserted again by the same walk from its
 * key's twin home, unless that is the same line (under pairs it never is);
 * *n_twins counts those second records. */
__global__ __launch_bounds__(256) void lines_build_kernel(const packed_bucket *__restrict__ src, uint64_t num_sigs,
                                                          uint64_t src_magic, packed_bucket *lines, uint64_t n_lines,
                                                          uint64_t line_magic, uint32_t home_w, uint32_t *overflow,
                                                          unsigned long long *n_twins)
{
    const uint64_t NB = 4 * n_lines;
    const bool twins = home_twins_of(home_w);
    uint64_t made = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < num_sigs;
         b += (uint64_t)gridDim.x * blockDim.x) {
        const packed_bucket e = src[b];
        const uint64_t key = e.lo & PACK_KEY_MASK;
        if (key > MAX_ENCODED)
            continue;
        bool first = true;
        for (uint64_t x = mod_by(key, num_sigs, src_magic); x != b; x = x + 1 == num_sigs ? 0 : x + 1) {
            const uint64_t k2 = src[x].lo & PACK_KEY_MASK;
            if (k2 == key || k2 > MAX_ENCODED) {
                first = false;
                break;
            }
        }
        if (!first)
            continue;
        uint64_t home, other;
        key_homes(key, n_lines, line_magic, home_w, home, other);
        for (int copy = 0; copy < (other != home ? 2 : 1); copy++) {
            uint64_t x = (copy ? other : home) * 4;
            bool placed = false;
            for (uint64_t n = 0; n < NB && !placed; n++) {
                const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(&lines[x].lo),
                                                          (unsigned long long)EMPTY_KEY, (unsigned long long)e.lo);
                if (prev == (unsigned long long)EMPTY_KEY) {
                    lines[x].hi = e.hi;
                    placed = true;
                }
                x = x + 1 == NB ? 0 : x + 1;
            }
            if (!placed)
                atomicOr(overflow, 1u);
            made += copy && placed;
        }
    }
    if (twins) {
        for (int o = 32; o > 0; o >>= 1)
            made += __shfl_xor(made, o);
        if (lane_id() == 0 && made)
            atomicAdd(n_twins, (unsigned long long)made);
    }
}

/* The overflow marks of a finished line index (kgx_line_home.h): every record
 * that lies past its key's home line sets its key's mark on each line from
 * the home to the one before its own, the lines its insertion passed.  A
 * kernel of its own, after the inserts: the inserter's plain store of `hi`
 * would race with another key's OR.  SCRATCH: the same marks into a separate
 * array instead, 16 bits per line, two lines per word (kgx_image_line_stats
 * compares the two).
 *
 * `twins`: a key has two homes and a record does not say which one it was
 * inserted from, so each record walks from both homes of its key and marks
 * every line before the first one that holds the key (its own line at the
 * latest: only full lines are passed, and no record ever leaves).  Both copies
 * of a key do the same two walks; the ORs are idempotent.  The counts are
 * kept in halves so that they stay per key: a key with one home line adds 2
 * to stats[0] and 2 to stats[1] if it lies past that line; each of the two
 * records of a key with two home lines adds 1 to stats[0] and 1 to stats[1]
 * for each home whose line does not hold the key.  kgx_image_line_stats
 * halves both sums.  Without twins both are counted whole, as they were. */
template <bool SCRATCH>
__global__ __launch_bounds__(256) void lines_mark_kernel(packed_bucket *lines, uint64_t n_lines, uint64_t line_magic,
                                                         uint32_t home_w, uint32_t *scratch,
                                                         unsigned long long *stats)
{
    const uint64_t NB = 4 * n_lines;
    const bool twins = home_twins_of(home_w);
    uint64_t stored = 0, past = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; b < NB; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = lines[b].lo & PACK_KEY_MASK;
        if (key > MAX_ENCODED)
            continue;
        const uint64_t own = b / 4;
        uint64_t home, other;
        key_homes(key, n_lines, line_magic, home_w, home, other);
        const uint32_t n_homes = other != home ? 2 : 1;
        const uint32_t unit = twins && n_homes == 1 ? 2 : 1;
        stored += unit;
        const uint32_t g = line_mark(key);
        for (uint32_t h = 0; h < n_homes; h++) {
            uint64_t l = h ? other : home;
            bool passed = false;
            while (l != own) {
                if (twins) { /* the other copy may lie before this one on the chain */
                    bool holds = false;
                    for (uint32_t r = 0; r < 4; r++)
                        holds |= (lines[4 * l + r].lo & PACK_KEY_MASK) == key;
                    if (holds)
                        break;
                }
                passed = true;
                if (SCRATCH)
                    atomicOr(scratch + (l >> 1), 1u << (g + 16u * (uint32_t)(l & 1)));
                else
                    atomicOr(reinterpret_cast<unsigned long long *>(&lines[4 * l + mark_record(g)].hi),
                             1ull << (32 + mark_bit_w(g)));
                l = l + 1 == n_lines ? 0 : l + 1;
            }
            past += passed ? unit : 0;
        }
    }
    if (SCRATCH) {
        for (int o = 32; o > 0; o >>= 1) {
            stored += __shfl_xor(stored, o);
            past += __shfl_xor(past, o);
        }
        if (lane_id() == 0 && stored) {
            atomicAdd(stats + 0, (unsigned long long)stored);
            atomicAdd(stats + 1, (unsigned long long)past);
        }
    }
}

/* kgx_image_line_stats, after lines_mark_kernel<true>: per line, whether it
 * is full, its marks, and their difference from the marks the stored records
 * call for (scratch): missing = called for and clear, unjustified = set and
 * not called for */
__global__ __launch_bounds__(256) void lines_stats_kernel(const packed_bucket *__restrict__ lines, uint64_t n_lines,
                                                          const uint32_t *__restrict__ scratch,
                                                          unsigned long long *stats)
{
    uint64_t v[5] = {0, 0, 0, 0, 0}; /* full lines, marked lines, bits, missing, unjustified */
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l < n_lines;
         l += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t have = 0, full = 1;
        for (uint32_t r = 0; r < 4; r++) {
            const packed_bucket e = lines[4 * l + r];
            full &= (e.lo & PACK_KEY_MASK) <= MAX_ENCODED;
            have |= (uint32_t)(e.hi >> 60) << (4 * r);
        }
        const uint32_t want = scratch[l >> 1] >> (16u * (uint32_t)(l & 1)) & 0xFFFFu;
        v[0] += full;
        v[1] += have != 0;
        v[2] += (uint32_t)__popc(have);
        v[3] += (uint32_t)__popc(want & ~have);
        v[4] += (uint32_t)__popc(have & ~want);
    }
    for (int k = 0; k < 5; k++) {
        for (int o = 32; o > 0; o >>= 1)
            v[k] += __shfl_xor(v[k], o);
        if (lane_id() == 0 && v[k])
            atomicAdd(stats + 2 + k, (unsigned long long)v[k]);
    }
}

__global__ __launch_bounds__(256) void fill_empty_kernel(packed_bucket *t, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        t[i].lo = EMPTY_KEY;
        t[i].hi = 0;
    }
}

/* *count += the PACKED16 table's stored keys */
static hipError_t launch_count_keys(const packed_bucket *t, uint64_t n, unsigned long long *count, hipStream_t stream)
{
    hipLaunchKernelGGL(count_keys_kernel, dim3(4096), dim3(256), 0, stream, t, n, count);
    return hipGetLastError();
}

/* the line index of a PACKED16 table (lines_build_kernel): 4 * n_lines
 * buckets, homes by the home word `home` (key_homes, kgx_line_home.h);
 * *overflow |= 1 when some record found no bucket; with the word's marks bit:
 * then the overflow marks, by lines_mark_kernel; with its twins bit (minimizer
 * home with marks only): every key with two home lines is stored under both,
 * *n_twins += those second records */
static hipError_t launch_lines_build(const packed_bucket *src, uint64_t num_sigs, packed_bucket *lines,
                                     uint64_t n_lines, uint32_t home, uint32_t *overflow,
                                     unsigned long long *n_twins, hipStream_t stream)
{
    const uint64_t line_magic = mod_magic(home_magic_lines(n_lines, home));
    hipLaunchKernelGGL(fill_empty_kernel, dim3(8192), dim3(256), 0, stream, lines, 4 * n_lines);
    hipLaunchKernelGGL(lines_build_kernel, dim3(8192), dim3(256), 0, stream, src, num_sigs, mod_magic(num_sigs), lines,
                       n_lines, line_magic, home, overflow, n_twins);
    if (home_marks_of(home))
        hipLaunchKernelGGL(lines_mark_kernel<false>, dim3(8192), dim3(256), 0, stream, lines, n_lines, line_magic,
                           home, nullptr, nullptr);
    return hipGetLastError();
}

/* kgx_image_line_stats: stats[0..7) += stored keys, records past their
 * home line (both twice over an index with twins, see lines_mark_kernel),
 * full lines, lines with a mark, mark bits set, missing and unjustified
 * marks; scratch: (n_lines + 1) / 2 zeroed words */
static hipError_t launch_lines_stats(const packed_bucket *lines, uint64_t n_lines, uint32_t home, uint32_t *scratch,
                                     unsigned long long *stats, hipStream_t stream)
{
    hipLaunchKernelGGL(lines_mark_kernel<true>, dim3(8192), dim3(256), 0, stream, const_cast<packed_bucket *>(lines),
                       n_lines, mod_magic(home_magic_lines(n_lines, home)), home, scratch, stats);
    hipLaunchKernelGGL(lines_stats_kernel, dim3(8192), dim3(256), 0, stream, lines, n_lines, scratch, stats);
    return hipGetLastError();
}

hipError_t launch_pack(const kgx_sig_kmer *table, packed_bucket *packed, uint64_t n,
                       uint32_t *not_packable, hipStream_t stream)
{
    hipLaunchKernelGGL(pack_kernel, dim3(8192), dim3(256), 0, stream, table, packed, n, not_packable);
    return hipGetLastError();
}

hipError_t launch_unpack(const packed_bucket *packed, kgx_sig_kmer *out, uint64_t n,
                         hipStream_t stream)
{
    hipLaunchKernelGGL(unpack_kernel, dim3(8192), dim3(256), 0, stream, packed, out, n);
    return hipGetLastError();
}

}  // namespace kgx

using namespace kgx;

/* ------------------------------------------------------------------------ */
/* the line index of an image (kgx.h)                                        */
/* ------------------------------------------------------------------------ */

int kgx_image_set_line_index(kgx_image *img, uint32_t keys_per_64_lines)
{
    if (!img)
        return fail(KGX_EINVAL, "null image");
    if (keys_per_64_lines > 255)
        return fail(KGX_EINVAL, "line index load: 0 (none) or 1 .. 255 keys per 64 lines");
    /* the home of a key in this index: KGX_LINE_HOME 1 = the minimizer home
     * (the default), 0 = key mod n_lines (kgx_line_home.h); read at each
     * call, a property of the index it builds */
    bool minimizer = true;
    if (int rc = env_switch("KGX_LINE_HOME", "mod", "minimizer", minimizer))
        return rc;
    const uint32_t home_mode = minimizer ? LINE_HOME_MINIMIZER : LINE_HOME_MOD;
    /* overflow marks on the index's full lines, which end an absent key's
     * chain in one line (kgx_line_home.h): KGX_LINE_MARKS 1 (the default)
     * builds them, 0 builds none; read at each call like KGX_LINE_HOME */
    bool marks = true;
    if (int rc = env_switch("KGX_LINE_MARKS", "none", "marks", marks))
        return rc;
    /* twin records, which let two neighbouring windows always share a line
     * (kgx_line_home.h): KGX_LINE_TWINS 1 (the default) builds them where the
     * rule of kgx.h allows, 0 builds none; read at each call like the two above */
    bool twins = minimizer && marks && keys_per_64_lines <= KGX_LINE_TWINS_MAX_LOAD;
    if (int rc = env_switch("KGX_LINE_TWINS", "none", "twins", twins))
        return rc;
    /* pairs: a 7-mer's two roles homed on the halves of a 128-byte block
     * (kgx_line_home.h), only where twins are built: KGX_LINE_PAIRS 1 turns
     * them on, 0 off; unset they are on for an index of more than
     * KGX_LINE_PAIRS_MIN_LINES lines (kgx.h); read at each call like the rest */
    bool pairs = twins;
    if (int rc = env_switch("KGX_LINE_PAIRS", "twins on one line", "pairs", pairs))
        return rc;
    const char *pairs_env = std::getenv("KGX_LINE_PAIRS");
    const bool pairs_by_size = !pairs_env || !*pairs_env;
    /* the service's workgroups hold the probe table's address */
    const auto hold = svc_shutdown_hold(img);
    HIP_TRY(hipSetDevice(img->device));
    HIP_TRY(hipDeviceSynchronize());
    drop_line_index(img);
    if (!keys_per_64_lines)
        return KGX_OK;
    if (img->layout != KGX_LAYOUT_PACKED16)
        return fail(KGX_EINVAL, "a line index needs a PACKED16 image");
    unsigned long long *d_count = nullptr; /* stored keys, twin records, the overflow flag */
    uint32_t *d_over = nullptr;
    HIP_TRY(hipMalloc(&d_count, 24));
    d_over = reinterpret_cast<uint32_t *>(d_count + 2);
    hipError_t e = hipMemset(d_count, 0, 24);
    if (e == hipSuccess)
        e = launch_count_keys(img->d_packed, img->num_sigs, d_count, nullptr);
    unsigned long long n_keys = 0;
    if (e == hipSuccess)
        e = hipMemcpy(&n_keys, d_count, 8, hipMemcpyDeviceToHost);
    /* lines: n_keys * 64 / load, odd and prime to 5 (keys are base-20 codes) */
    uint64_t n_lines = std::max<uint64_t>(1, (uint64_t)(((unsigned __int128)n_keys * 64 + keys_per_64_lines - 1) /
                                                        keys_per_64_lines));
    while (n_lines % 2 == 0 || n_lines % 5 == 0)
        n_lines++;
    pairs = pairs && n_lines >= 3 && (!pairs_by_size || n_lines > KGX_LINE_PAIRS_MIN_LINES);
    const uint32_t home = home_word(2u, home_mode, marks, twins, pairs);
    packed_bucket *lines = nullptr;
    if (e == hipSuccess && (4 * n_lines >= (1ull << 40) || hipMalloc(&lines, 4 * n_lines * sizeof(packed_bucket)) != hipSuccess)) {
        (void)hipGetLastError();
        (void)hipFree(d_count);
        return fail(KGX_ENOMEM, "no room for the line index (" + std::to_string(4 * n_lines * 16) + " B)");
    }
    uint32_t over = 0;
    unsigned long long n_twins = 0;
    if (e == hipSuccess)
        e = launch_lines_build(img->d_packed, img->num_sigs, lines, n_lines, home, d_over, d_count + 1, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&over, d_over, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(&n_twins, d_count + 1, 8, hipMemcpyDeviceToHost);
    (void)hipFree(d_count);
    if (e != hipSuccess || over) {
        if (lines)
            (void)hipFree(lines);
        return fail(KGX_EDEVICE, e != hipSuccess ? std::string("line index: ") + hipGetErrorString(e)
                                                 : std::string("line index: a record found no bucket"));
    }
    img->lines.records = lines;
    img->lines.n_lines = n_lines;
    img->lines.home = home_mode;
    img->lines.marks = marks;
    img->lines.twins = twins;
    img->lines.pairs = pairs;
    img->lines.n_twins = n_twins;
    img->lines.load = keys_per_64_lines;
    return KGX_OK;
}

uint64_t kgx_image_line_count(const kgx_image *img) { return img ? img->lines.n_lines : 0; }
uint32_t kgx_image_line_home(const kgx_image *img) { return img ? img->lines.home : 0; }
uint64_t kgx_image_line_twins(const kgx_image *img) { return img ? img->lines.n_twins : 0; }
uint32_t kgx_image_line_pairs(const kgx_image *img) { return img && img->lines.pairs ? 1u : 0u; }

int kgx_image_line_stats(const kgx_image *img, uint64_t out[8])
{
    if (!img || !out)
        return fail(KGX_EINVAL, "null image or output");
    const LineIndex &li = img->lines;
    if (!li)
        return fail(KGX_EINVAL, "the image has no line index");
    HIP_TRY(hipSetDevice(img->device));
    /* the marks the stored records call for, 16 bits a line, and 8 counters */
    const uint64_t words = (li.n_lines + 1) / 2;
    uint32_t *d_scratch = nullptr;
    if (hipMalloc(&d_scratch, words * 4 + 64) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KGX_ENOMEM, "no room for the line statistics (" + std::to_string(words * 4) + " B)");
    }
    unsigned long long *d_stats = reinterpret_cast<unsigned long long *>(d_scratch);
    hipError_t e = hipMemset(d_scratch, 0, words * 4 + 64);
    if (e == hipSuccess)
        e = launch_lines_stats(li.records, li.n_lines, li.home_word(), d_scratch + 16, d_stats, nullptr);
    unsigned long long h[8] = {};
    if (e == hipSuccess)
        e = hipMemcpy(h, d_stats, sizeof h, hipMemcpyDeviceToHost);
    (void)hipFree(d_scratch);
    if (e != hipSuccess)
        return fail(KGX_EDEVICE, std::string("line statistics: ") + hipGetErrorString(e));
    for (int i = 0; i < 8; i++)
        out[i] = h[i];
    if (li.twins) { /* counted in halves, per key (lines_mark_kernel) */
        out[0] /= 2;
        out[1] /= 2;
    }
    return KGX_OK;
}
