/*
 * line_share_probe -- what a repeated line costs the cooperative line read.
 *
 * The line probe reads the table as the quads of a wave instruction do: 4
 * lanes per aligned 64-B line, 16 B each, 16 random lines per instruction,
 * ILP instructions in flight per wave.  Its ceiling is the chip's rate of
 * random line requests.  This program asks what that ceiling charges when a
 * share of the quads want the line of the quad before them (neighbouring
 * windows homed on one line):
 *
 *   form a   the repeating quad issues its load anyway (same address as its
 *            neighbour's, same instruction)
 *   form b   the repeating quad issues no load and takes its 16 B from lane
 *            - 4 once the neighbour's load is back
 *
 * Odd quads repeat the even quad before them with probability 2 * share, so
 * runs of one line are never longer than two quads.  A "window" is one quad
 * of one instruction, repeated or not.  One JSON object on stdout.
 *
 *   halves   every even quad reads line 2k and the odd quad after it line
 *            2k + 1 of one random aligned 128-B block (a 7-mer's block under
 *            the pairs layout): 8 lanes on one block in one instruction.  It
 *            is timed in alternation with form a at share 1/2, HALVES_REPEATS
 *            times; a block there stands against a distinct line here, and
 *            "halves_over_shared" is blocks/s over distinct lines/s.
 *
 *   hipcc -O3 --offload-arch=gfx950 tools/line_share_probe.cpp -o tools/line_share_probe
 *   tools/line_share_probe [GiB of buffer, default 64] [device, default 0]
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x)                                                                               \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

constexpr int ILP = 8;       /* the probe's instructions per 128-window tile */
constexpr uint32_t ROUNDS = 8;

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* x % n for x < 2^35, m = floor((2^64-1)/n) */
__device__ __forceinline__ uint64_t mod_by(uint64_t x, uint64_t n, uint64_t m)
{
    const uint64_t r = x - __umul64hi(x, m) * n;
    return r >= n ? r - n : r;
}

/* share1024: odd quads repeat when their coin (0..1023) is below it */
template <bool SKIP>
__global__ __launch_bounds__(256) void share_kernel(const uint4 *__restrict__ base, uint64_t n_lines, uint64_t magic,
                                                    uint32_t share1024, uint64_t *__restrict__ sink)
{
    const uint64_t gw = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 2, c = lane & 3u;
    uint64_t acc = 0;
    for (uint32_t r = 0; r < ROUNDS; r++) {
        uint64_t line[ILP];
        bool rep[ILP];
#pragma unroll
        for (int k = 0; k < ILP; k++) {
            const uint64_t at = (gw * ROUNDS + r) * ILP + k;
            const uint64_t h = mix64(at * 16 + q);
            rep[k] = (q & 1u) && (uint32_t)(h >> 40 & 1023u) < share1024;
            const uint64_t src = rep[k] ? mix64(at * 16 + q - 1) : h;
            line[k] = mod_by(src & ((1ull << 35) - 1), n_lines, magic);
        }
        uint4 d[ILP];
#pragma unroll
        for (int k = 0; k < ILP; k++)
            if (!SKIP || !rep[k])
                d[k] = base[line[k] * 4 + c];
#pragma unroll
        for (int k = 0; k < ILP; k++) {
            uint4 v = d[k];
            if (SKIP) {
                const uint32_t x = (uint32_t)__shfl_up((int)d[k].x, 4), y = (uint32_t)__shfl_up((int)d[k].y, 4);
                const uint32_t z = (uint32_t)__shfl_up((int)d[k].z, 4), w = (uint32_t)__shfl_up((int)d[k].w, 4);
                v.x = rep[k] ? x : d[k].x;
                v.y = rep[k] ? y : d[k].y;
                v.z = rep[k] ? z : d[k].z;
                v.w = rep[k] ? w : d[k].w;
            }
            acc += ((uint64_t)v.y << 32 | v.x) ^ ((uint64_t)v.w << 32 | v.z);
        }
    }
    sink[(uint64_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

/* quads 2i and 2i + 1 read the two halves of one random aligned 128-B block */
__global__ __launch_bounds__(256) void halves_kernel(const uint4 *__restrict__ base, uint64_t n_blocks, uint64_t magic,
                                                     uint64_t *__restrict__ sink)
{
    const uint64_t gw = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u, q = lane >> 2, c = lane & 3u;
    uint64_t acc = 0;
    for (uint32_t r = 0; r < ROUNDS; r++) {
        uint64_t line[ILP];
#pragma unroll
        for (int k = 0; k < ILP; k++) {
            const uint64_t at = (gw * ROUNDS + r) * ILP + k;
            const uint64_t h = mix64(at * 16 + (q & ~1u));
            line[k] = 2 * mod_by(h & ((1ull << 35) - 1), n_blocks, magic) + (q & 1u);
        }
        uint4 d[ILP];
#pragma unroll
        for (int k = 0; k < ILP; k++)
            d[k] = base[line[k] * 4 + c];
#pragma unroll
        for (int k = 0; k < ILP; k++)
            acc += ((uint64_t)d[k].y << 32 | d[k].x) ^ ((uint64_t)d[k].w << 32 | d[k].z);
    }
    sink[(uint64_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

constexpr int HALVES_REPEATS = 5;

int main(int argc, char **argv)
{
    const uint64_t gib = argc > 1 ? strtoull(argv[1], nullptr, 10) : 64;
    const int device = argc > 2 ? atoi(argv[2]) : 0;
    CHECK(hipSetDevice(device));
    uint64_t n_lines = (gib << 30) / 64;
    while (n_lines % 2 == 0 || n_lines % 5 == 0)
        n_lines--;
    if (n_lines < 1 || n_lines >= (1ull << 35)) {
        fprintf(stderr, "buffer of %llu GiB out of range\n", (unsigned long long)gib);
        return 1;
    }
    const uint64_t magic = ~0ull / n_lines;
    const uint32_t blocks = 8192;
    uint4 *buf = nullptr;
    uint64_t *sink = nullptr;
    CHECK(hipMalloc(&buf, n_lines * 64));
    CHECK(hipMalloc(&sink, (uint64_t)blocks * 256 * 8));
    CHECK(hipMemset(buf, 0x5a, n_lines * 64));
    CHECK(hipDeviceSynchronize());
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    const double windows = (double)blocks * 4 * 16 * ILP * ROUNDS;
    const struct {
        const char *name;
        uint32_t share1024; /* of the odd quads: twice the share of all quads */
        double share;
    } shares[] = {{"0", 0, 0.0}, {"1/3", 683, 1.0 / 3}, {"1/2", 1024, 0.5}};
    printf("{\"tool\": \"line_share_probe\", \"buffer_GiB\": %llu, \"lines\": %llu, \"ilp\": %d, "
           "\"windows_per_launch\": %.0f, \"samples\": 9, \"results\": [",
           (unsigned long long)gib, (unsigned long long)n_lines, ILP, windows);
    bool first = true;
    for (const auto &s : shares) {
        for (int form = 0; form < 2; form++) {
            std::vector<float> ms;
            for (int it = 0; it < 11; it++) { /* two warm-up launches */
                CHECK(hipEventRecord(e0, nullptr));
                if (form == 0)
                    hipLaunchKernelGGL(share_kernel<false>, dim3(blocks), dim3(256), 0, nullptr, buf, n_lines, magic,
                                       s.share1024, sink);
                else
                    hipLaunchKernelGGL(share_kernel<true>, dim3(blocks), dim3(256), 0, nullptr, buf, n_lines, magic,
                                       s.share1024, sink);
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e1, nullptr));
                CHECK(hipEventSynchronize(e1));
                float t = 0;
                CHECK(hipEventElapsedTime(&t, e0, e1));
                if (it >= 2)
                    ms.push_back(t);
            }
            std::sort(ms.begin(), ms.end());
            const double med = ms[ms.size() / 2];
            printf("%s{\"share\": \"%s\", \"form\": \"%s\", \"median_ms\": %.4f, \"min_ms\": %.4f, \"max_ms\": %.4f, "
                   "\"windows_per_s\": %.4g, \"distinct_lines_per_s\": %.4g}",
                   first ? "" : ", ", s.name, form == 0 ? "a_load_anyway" : "b_skip_and_shift", med, ms.front(),
                   ms.back(), windows / (med * 1e-3), windows * (1.0 - s.share) / (med * 1e-3));
            first = false;
        }
    }
    /* the gate of the pairs layout: halves against the shared line, alternated */
    const uint64_t n_blocks = n_lines >> 1, magic_blocks = ~0ull / n_blocks;
    printf("], \"halves_blocks\": %llu, \"halves\": [", (unsigned long long)n_blocks);
    for (int rep = 0; rep < HALVES_REPEATS; rep++) {
        double med[2], lo[2], hi[2];
        for (int form = 0; form < 2; form++) {
            std::vector<float> ms;
            for (int it = 0; it < 11; it++) {
                CHECK(hipEventRecord(e0, nullptr));
                if (form == 0)
                    hipLaunchKernelGGL(share_kernel<false>, dim3(blocks), dim3(256), 0, nullptr, buf, n_lines, magic,
                                       1024u, sink);
                else
                    hipLaunchKernelGGL(halves_kernel, dim3(blocks), dim3(256), 0, nullptr, buf, n_blocks,
                                       magic_blocks, sink);
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e1, nullptr));
                CHECK(hipEventSynchronize(e1));
                float t = 0;
                CHECK(hipEventElapsedTime(&t, e0, e1));
                if (it >= 2)
                    ms.push_back(t);
            }
            std::sort(ms.begin(), ms.end());
            med[form] = ms[ms.size() / 2];
            lo[form] = ms.front();
            hi[form] = ms.back();
        }
        printf("%s{\"repeat\": %d, \"shared_median_ms\": %.4f, \"shared_min_ms\": %.4f, \"shared_max_ms\": %.4f, "
               "\"shared_distinct_lines_per_s\": %.4g, \"halves_median_ms\": %.4f, \"halves_min_ms\": %.4f, "
               "\"halves_max_ms\": %.4f, \"halves_blocks_per_s\": %.4g, \"halves_over_shared\": %.4f}",
               rep ? ", " : "", rep, med[0], lo[0], hi[0], windows * 0.5 / (med[0] * 1e-3), med[1], lo[1], hi[1],
               windows * 0.5 / (med[1] * 1e-3), med[0] / med[1]);
    }
    printf("]}\n");
    CHECK(hipFree(buf));
    CHECK(hipFree(sink));
    return 0;
}
