/*
 * kgx_runtime.cpp -- host side of the C ABI (include/kgx.h): image loading
 * and replication into HBM, per-thread contexts, batch orchestration, host
 * OTU tallies.
 *
 * Replaces KmerImage (kmer_image.cc:41-108) and the per-sequence loop of
 * KmerGuts::process_aa_seq (kguts.cc:888-908) with batched HIP launches.
 */
#include <hip/hip_runtime.h>
#include <sched.h>

#include <algorithm>
#include <cerrno>
#include <ctime>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <atomic>
#include <fcntl.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "kgx_rt.h"

using namespace kgx;

namespace kgx {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg)
{
    g_last_error = msg;
    return code;
}

bool is_gfx950(int dev)
{
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
        return false;
    return std::strncmp(prop.gcnArchName, "gfx950", 6) == 0;
}

namespace {

int wait_mode_from_env(uint32_t *us)
{
    *us = 20;
    const char *e = std::getenv("KGX_HOST_WAIT");
    if (!e)
        return KGX_WAIT_SPIN;
    const std::string v(e);
    if (v.rfind("sleep", 0) == 0) {
        if (v.size() > 6 && v[5] == ':')
            *us = (uint32_t)std::max(1, std::atoi(v.c_str() + 6));
        return KGX_WAIT_SLEEP;
    }
    return v == "block" ? KGX_WAIT_BLOCK : KGX_WAIT_SPIN;
}

uint32_t g_env_wait_us = 20;

void sleep_us(uint32_t us)
{
    timespec ts{0, (long)us * 1000};
    nanosleep(&ts, nullptr);
}

}  // namespace

std::atomic<int> g_host_wait_mode{wait_mode_from_env(&g_env_wait_us)};
std::atomic<uint32_t> g_host_wait_us{g_env_wait_us};

hipError_t host_wait(hipStream_t s)
{
    const int mode = g_host_wait_mode.load(std::memory_order_relaxed);
    if (mode == KGX_WAIT_SLEEP) {
        const uint32_t us = g_host_wait_us.load(std::memory_order_relaxed);
        for (;;) {
            const hipError_t q = hipStreamQuery(s);
            if (q != hipErrorNotReady)
                return q;
            sleep_us(us);
        }
    }
    if (mode == KGX_WAIT_BLOCK) {
        /* one blocking-sync event per thread and device, never destroyed (a
         * thread_local destructor must not call the runtime at exit, §10) */
        thread_local hipEvent_t ev[64] = {};
        int dev = 0;
        hipError_t e = hipStreamGetDevice(s, &dev);
        if (e != hipSuccess || dev < 0 || dev >= 64)
            return e != hipSuccess ? e : hipStreamSynchronize(s);
        if (!ev[dev]) {
            int cur = 0;
            if ((e = hipGetDevice(&cur)) != hipSuccess || (cur != dev && (e = hipSetDevice(dev)) != hipSuccess))
                return e;
            e = hipEventCreateWithFlags(&ev[dev], hipEventDisableTiming | hipEventBlockingSync);
            if (cur != dev)
                (void)hipSetDevice(cur);
            if (e != hipSuccess) {
                ev[dev] = nullptr;
                return e;
            }
        }
        if ((e = hipEventRecord(ev[dev], s)) != hipSuccess)
            return e;
        return hipEventSynchronize(ev[dev]);
    }
    return hipStreamSynchronize(s);
}

hipError_t host_wait_word(const volatile uint32_t *done, uint32_t token, hipStream_t s)
{
    const int mode = g_host_wait_mode.load(std::memory_order_relaxed);
    if (mode == KGX_WAIT_BLOCK)
        return host_wait(s); /* the stream drains after the word's store */
    const uint32_t us = g_host_wait_us.load(std::memory_order_relaxed);
    const auto w0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 1; *done != token; spin++) {
        if (mode == KGX_WAIT_SLEEP || (spin & 255u) == 0) { /* a fault or a lost store still ends the wait */
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess)
                break;
            if (q != hipErrorNotReady)
                return q;
            if (mode == KGX_WAIT_SLEEP)
                sleep_us(us);
            /* past 50 us of spinning the CPU goes to whoever else is
             * runnable (a server's other workers, its socket threads) */
            else if (std::chrono::steady_clock::now() - w0 > std::chrono::microseconds(50))
                sched_yield();
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return hipSuccess;
}

}  // namespace kgx

/* [p, p + n) lies in one pinned, device-mapped host allocation */
bool kgx::host_pinned_range(const void *p, uint64_t n, const void **device_address)
{
    if (!p || n == 0)
        return false;
    hipPointerAttribute_t a{}, b{};
    const char *first = static_cast<const char *>(p), *last = first + n - 1;
    if (hipPointerGetAttributes(&a, first) != hipSuccess || a.type != hipMemoryTypeHost || !a.devicePointer ||
        hipPointerGetAttributes(&b, last) != hipSuccess || b.type != hipMemoryTypeHost || !b.devicePointer) {
        (void)hipGetLastError(); /* an unregistered pointer is not an error here */
        return false;
    }
    const bool one = static_cast<const char *>(b.devicePointer) - static_cast<const char *>(a.devicePointer) ==
                     (std::ptrdiff_t)(n - 1);
    if (one && device_address)
        *device_address = a.devicePointer;
    return one;
}


extern "C" {

const char *kgx_version(void) { return "close_kmers_amd 0.1 (gfx950)"; }

const char *kgx_last_error(void) { return g_last_error.c_str(); }

const char *kgx_strerror(int code)
{
    switch (code) {
    case KGX_OK: return "ok";
    case KGX_EINVAL: return "invalid argument";
    case KGX_EIO: return "i/o error";
    case KGX_EFORMAT: return "image format mismatch";
    case KGX_ENOMEM: return "out of memory";
    case KGX_EDEVICE: return "device error";
    case KGX_ERANGE: return "out of supported range";
    case KGX_EFULL: return "hash table half full";
    case KGX_EBUSY: return "call service busy or not applicable";
    default: return "unknown error";
    }
}

int kgx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    int good = 0;
    for (int d = 0; d < n; d++)
        good += is_gfx950(d) ? 1 : 0;
    return good;
}

int kgx_set_host_wait(int mode, uint32_t poll_us)
{
    if (mode != KGX_WAIT_SPIN && mode != KGX_WAIT_SLEEP && mode != KGX_WAIT_BLOCK)
        return fail(KGX_EINVAL, "host wait mode: KGX_WAIT_SPIN, KGX_WAIT_SLEEP or KGX_WAIT_BLOCK");
    g_host_wait_us.store(poll_us ? std::min<uint32_t>(poll_us, 100000) : 20u);
    g_host_wait_mode.store(mode);
    return KGX_OK;
}

int kgx_get_host_wait(uint32_t *poll_us)
{
    if (poll_us)
        *poll_us = g_host_wait_us.load();
    return g_host_wait_mode.load();
}

int kgx_params_default(kgx_params *p)
{
    if (!p)
        return fail(KGX_EINVAL, "null params");
    /* set_default_parameters, kguts.cc:236-242 */
    p->order_constraint = 0;
    p->min_hits = 5;
    p->min_weighted_hits = 0;
    p->max_gap = 200;
    return KGX_OK;
}

int kgx_params_parse(kgx_params *p, const char *const *names, const char *const *values, size_t n)
{
    if (!p || (n && (!names || !values)))
        return fail(KGX_EINVAL, "null argument");
    kgx_params_default(p);
    /* set_parameters, kguts.cc:244-268: std::stoi; invalid_argument warns */
    for (size_t i = 0; i < n; i++) {
        int32_t *dst = nullptr;
        std::string k = names[i] ? names[i] : "";
        if (k == "order_constraint")
            dst = &p->order_constraint;
        else if (k == "min_hits")
            dst = &p->min_hits;
        else if (k == "min_weighted_hits")
            dst = &p->min_weighted_hits;
        else if (k == "max_gap")
            dst = &p->max_gap;
        if (!dst)
            continue;
        try {
            *dst = std::stoi(values[i] ? values[i] : "");
        } catch (const std::invalid_argument &) {
            std::fprintf(stderr, "Warning: invalid integer '%s' passed for parameter %s\n",
                         values[i] ? values[i] : "", k.c_str());
        } catch (const std::out_of_range &) {
            return fail(KGX_ERANGE, "parameter " + k + " out of int range");
        }
    }
    return KGX_OK;
}

/* ---- images ------------------------------------------------------------ */

/* an image on `device` with its resident table allocated in `layout`
 * (AOS24: the file's 24-B buckets; PACKED16: 16-B records, a replica of a
 * packed image, so no 24-B table is ever allocated for it) */
static int image_alloc(int device, uint64_t num_sigs, kgx_image **out, int layout = KGX_LAYOUT_AOS24)
{
    if (!out)
        return fail(KGX_EINVAL, "null output");
    if (num_sigs == 0)
        return fail(KGX_EFORMAT, "image with zero buckets");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(KGX_EDEVICE, "no such HIP device " + std::to_string(device));
    if (!is_gfx950(device))
        return fail(KGX_EDEVICE, "device " + std::to_string(device) + " is not gfx950");
    HIP_TRY(hipSetDevice(device));
    kgx_image *img = new kgx_image;
    img->device = device;
    img->num_sigs = num_sigs;
    hipError_t e = layout == KGX_LAYOUT_PACKED16 ? hipMalloc(&img->d_packed, num_sigs * sizeof(packed_bucket))
                                                  : hipMalloc(&img->d_table, num_sigs * sizeof(kgx_sig_kmer));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete img;
        return fail(KGX_ENOMEM, "hipMalloc of the image table failed: " +
                                    std::string(hipGetErrorString(e)));
    }
    img->layout = layout;
    *out = img;
    return KGX_OK;
}

/* AOS24 -> PACKED16 on the device; KGX_ERANGE (image unchanged) when some
 * stored bucket's payload does not fit the packed record */
static int image_pack(kgx_image *img)
{
    if (img->layout == KGX_LAYOUT_PACKED16)
        return KGX_OK;
    HIP_TRY(hipSetDevice(img->device));
    packed_bucket *p = nullptr;
    uint32_t *flag = nullptr;
    if (hipMalloc(&p, img->num_sigs * sizeof(packed_bucket)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KGX_ENOMEM, "no room for the packed table");
    }
    uint32_t bad = 0;
    hipError_t e = hipMalloc(&flag, sizeof(uint32_t));
    if (e == hipSuccess)
        e = hipMemset(flag, 0, sizeof(uint32_t));
    if (e == hipSuccess)
        e = launch_pack(img->d_table, p, img->num_sigs, flag, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&bad, flag, sizeof(bad), hipMemcpyDeviceToHost);
    if (flag)
        (void)hipFree(flag);
    if (e != hipSuccess || bad) {
        (void)hipFree(p);
        if (e != hipSuccess)
            return fail(KGX_EDEVICE, std::string("pack: ") + hipGetErrorString(e));
        return fail(KGX_ERANGE, "image payloads do not fit the packed layout");
    }
    (void)hipFree(img->d_table);
    img->d_table = nullptr;
    img->d_packed = p;
    img->layout = KGX_LAYOUT_PACKED16;
    return KGX_OK;
}

static int image_unpack(kgx_image *img)
{
    if (img->layout == KGX_LAYOUT_AOS24)
        return KGX_OK;
    HIP_TRY(hipSetDevice(img->device));
    kgx_sig_kmer *t = nullptr;
    if (hipMalloc(&t, img->num_sigs * sizeof(kgx_sig_kmer)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(KGX_ENOMEM, "no room for the 24-byte table");
    }
    hipError_t e = launch_unpack(img->d_packed, t, img->num_sigs, nullptr);
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipFree(t);
        return fail(KGX_EDEVICE, std::string("unpack: ") + hipGetErrorString(e));
    }
    (void)hipFree(img->d_packed);
    img->d_packed = nullptr;
    img->d_table = t;
    img->layout = KGX_LAYOUT_AOS24;
    return KGX_OK;
}

/* images are packed at load when they fit; otherwise they stay AOS24.
 * KGX_LINE_INDEX=<keys per 64 lines> also builds the line index of every
 * packed image at load (kgx_image_set_line_index; for programs that only
 * see images through the facade or the server) */
static int image_settle(kgx_image *img, kgx_image **out)
{
    int rc = image_pack(img);
    if (rc == KGX_EDEVICE) {
        kgx_image_close(img);
        return rc;
    }
    static const long line_load = [] {
        const char *e = std::getenv("KGX_LINE_INDEX");
        return e ? std::strtol(e, nullptr, 10) : 0L;
    }();
    if (line_load > 0 && img->layout == KGX_LAYOUT_PACKED16 &&
        (rc = kgx_image_set_line_index(img, (uint32_t)std::min(line_load, 255L)))) {
        kgx_image_close(img);
        return rc;
    }
    *out = img;
    return KGX_OK;
}

/* KmerImage::map_image_file validation, kmer_image.cc:128-147 */
static int validate_header(const kgx_image_header &h, uint64_t file_size)
{
    if (file_size != sizeof(kgx_sig_kmer) * h.num_sigs + sizeof(kgx_image_header))
        return fail(KGX_EFORMAT, "Version mismatch: file size does not match");
    if (h.version != 1)
        return fail(KGX_EFORMAT, "Version mismatch: file has " + std::to_string(h.version) +
                                     " code has 1");
    if (h.entry_size != sizeof(kgx_sig_kmer))
        return fail(KGX_EFORMAT, "Version mismatch: entry size " + std::to_string(h.entry_size));
    return KGX_OK;
}

/* A device destination of a file load: `dev` on `device`. */
struct LoadDst {
    char *dev;
    int device;
};

/* file bytes [off, off + total) -> every destination, by `threads` host
 * threads: thread t reads chunks t, t + threads, ... with pread into its own
 * two pinned buffers and copies each chunk up to every destination on that
 * destination's stream, so file reads (page cache or disk) run in parallel and
 * overlap the H2D copies, and a replicated image is read from the file once
 * (each device's copy runs on its own PCIe link).  The reference maps the file
 * with MAP_POPULATE instead (kmer_image.cc:66-77); the bytes are the same. */
static int load_file_range(int fd, uint64_t off, uint64_t total, const std::vector<LoadDst> &dsts, int threads,
                           size_t chunk)
{
    chunk = (size_t)std::max<uint64_t>(1, std::min<uint64_t>(chunk, total)); /* small files: small buffers */
    const uint64_t n_chunks = (total + chunk - 1) / chunk;
    threads = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)threads, n_chunks));
    const size_t D = dsts.size();
    std::atomic<bool> ok(true);
    std::string err;
    std::mutex err_mu;
    auto set_err = [&](const std::string &e) {
        std::lock_guard<std::mutex> g(err_mu);
        if (ok.exchange(false))
            err = e;
    };
    auto worker = [&](int t) {
        void *buf[2] = {nullptr, nullptr};
        std::vector<hipStream_t> st(D, nullptr);
        std::vector<hipEvent_t> ev(2 * D, nullptr); /* ev[k * D + d]: buffer k's copy to dst d */
        bool used[2] = {false, false};
        bool setup = hipSetDevice(dsts[0].device) == hipSuccess && hipHostMalloc(&buf[0], chunk, hipHostMallocPortable) == hipSuccess &&
                     hipHostMalloc(&buf[1], chunk, hipHostMallocPortable) == hipSuccess;
        for (size_t d = 0; setup && d < D; d++) {
            setup = hipSetDevice(dsts[d].device) == hipSuccess &&
                    hipStreamCreateWithFlags(&st[d], hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&ev[d], hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&ev[D + d], hipEventDisableTiming) == hipSuccess;
        }
        if (!setup) {
            set_err("pinned staging allocation failed");
        } else {
            int k = 0;
            for (uint64_t c = (uint64_t)t; c < n_chunks && ok.load(); c += (uint64_t)threads, k ^= 1) {
                const uint64_t at = c * chunk;
                const size_t n = (size_t)std::min<uint64_t>(chunk, total - at);
                bool waited = true;
                for (size_t d = 0; used[k] && d < D; d++)
                    waited = waited && hipEventSynchronize(ev[k * D + d]) == hipSuccess;
                if (!waited) {
                    set_err("staging copy failed");
                    break;
                }
                size_t got = 0;
                while (got < n) {
                    const ssize_t r = pread(fd, static_cast<char *>(buf[k]) + got, n - got, (off_t)(off + at + got));
                    if (r <= 0)
                        break;
                    got += (size_t)r;
                }
                if (got != n) {
                    set_err("short read");
                    break;
                }
                bool copied = true;
                for (size_t d = 0; copied && d < D; d++)
                    copied = hipSetDevice(dsts[d].device) == hipSuccess &&
                             hipMemcpyAsync(dsts[d].dev + at, buf[k], n, hipMemcpyHostToDevice, st[d]) == hipSuccess &&
                             hipEventRecord(ev[k * D + d], st[d]) == hipSuccess;
                if (!copied) {
                    set_err("H2D copy failed");
                    break;
                }
                used[k] = true;
            }
        }
        for (size_t d = 0; d < D; d++)
            if (st[d]) {
                (void)hipSetDevice(dsts[d].device);
                (void)hipStreamSynchronize(st[d]);
            }
        for (auto e : ev)
            if (e)
                (void)hipEventDestroy(e);
        for (int i = 0; i < 2; i++)
            if (buf[i])
                (void)hipHostFree(buf[i]);
        for (size_t d = 0; d < D; d++)
            if (st[d])
                (void)hipStreamDestroy(st[d]);
    };
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; t++)
        pool.emplace_back(worker, t);
    for (auto &th : pool)
        th.join();
    return ok.load() ? KGX_OK : fail(KGX_EIO, err);
}

/* reader threads of kgx_image_open: KGX_LOAD_THREADS, else one per GiB of
 * table up to 8 (each thread's pinned buffers cost more than they save on
 * small files: 768 MB loads at 8.2 GB/s with 1 thread, 3.3 GB/s with 8;
 * 25.8 GB at 22 GB/s with 8, profiles/r1s_image_load.json) */
static int load_threads(uint64_t bytes)
{
    const char *e = std::getenv("KGX_LOAD_THREADS");
    const int n = e ? std::atoi(e) : (int)std::min<uint64_t>(8, std::max<uint64_t>(1, bytes >> 30));
    return std::max(1, std::min(n, 64));
}

/* <dir>/kmer.table.mem_map: opened, stat'ed and its header validated
 * (kmer_image.cc:128-147); *fd stays open on success */
static int open_image_file(const char *dir, int *fd_out, kgx_image_header *h, std::string *path_out)
{
    const std::string path = std::string(dir) + "/kmer.table.mem_map";
    *path_out = path;
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd < 0)
        return fail(KGX_EIO, "open " + path + ": " + std::strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0) {
        ::close(fd);
        return fail(KGX_EIO, "stat " + path + " failed");
    }
    if (pread(fd, h, sizeof(*h), 0) != (ssize_t)sizeof(*h)) {
        ::close(fd);
        return fail(KGX_EFORMAT, "Version mismatch: file size does not match");
    }
    int rc = validate_header(*h, (uint64_t)st.st_size);
    if (rc) {
        ::close(fd);
        return rc;
    }
    *fd_out = fd;
    return KGX_OK;
}

int kgx_image_open(const char *dir, int device, kgx_image **out)
{
    if (!dir || !out)
        return fail(KGX_EINVAL, "null argument");
    return kgx_image_open_replicas(dir, &device, 1, out);
}

int kgx_image_open_replicas(const char *dir, const int *devices, uint32_t n, kgx_image **out)
{
    if (!dir || !out || !devices || n == 0)
        return fail(KGX_EINVAL, "null argument or no devices");
    for (uint32_t i = 0; i < n; i++)
        out[i] = nullptr;
    int fd = -1;
    kgx_image_header h;
    std::string path;
    int rc = open_image_file(dir, &fd, &h, &path);
    if (rc)
        return rc;
    std::vector<kgx_image *> imgs(n, nullptr);
    std::vector<LoadDst> dsts;
    auto close_all = [&]() {
        for (auto *im : imgs)
            kgx_image_close(im);
    };
    for (uint32_t i = 0; i < n; i++) {
        rc = image_alloc(devices[i], h.num_sigs, &imgs[i]);
        if (rc) {
            ::close(fd);
            close_all();
            return rc;
        }
        dsts.push_back({reinterpret_cast<char *>(imgs[i]->d_table), devices[i]});
    }
    rc = load_file_range(fd, sizeof(h), h.num_sigs * sizeof(kgx_sig_kmer), dsts,
                         load_threads(h.num_sigs * sizeof(kgx_sig_kmer)), 32ull << 20);
    ::close(fd);
    if (rc) {
        close_all();
        return fail(rc, "loading " + path + ": " + kgx_last_error());
    }
    /* every replica is packed on its own device at once */
    std::vector<int> rcs(n, KGX_OK);
    std::vector<std::string> errs(n);
    std::vector<std::thread> th;
    for (uint32_t i = 0; i < n; i++)
        th.emplace_back([&, i] {
            kgx_image *settled = nullptr;
            rcs[i] = image_settle(imgs[i], &settled); /* closes the image on failure */
            if (rcs[i])
                errs[i] = kgx_last_error();
            imgs[i] = rcs[i] ? nullptr : settled;
        });
    for (auto &t : th)
        t.join();
    for (uint32_t i = 0; i < n; i++)
        if (rcs[i]) {
            close_all();
            return fail(rcs[i], "replica on device " + std::to_string(devices[i]) + ": " + errs[i]);
        }
    for (uint32_t i = 0; i < n; i++)
        out[i] = imgs[i];
    return KGX_OK;
}

int kgx_image_replicate(const kgx_image *src, int device, kgx_image **out)
{
    if (!src || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = nullptr;
    kgx_image *img = nullptr;
    /* the source's resident layout only (a packed source never costs a 24-B
     * table on the target, not even briefly) */
    int rc = image_alloc(device, src->num_sigs, &img, src->layout);
    if (rc)
        return rc;
    hipError_t e = hipSuccess;
    /* device to device: xGMI between two GPUs (the runtime picks the path),
     * a device-local copy when both are the same GPU */
    e = hipMemcpyPeer(img->layout == KGX_LAYOUT_PACKED16 ? static_cast<void *>(img->d_packed) : img->d_table,
                      device, src->resident(), src->device, src->resident_bytes());
    if (e == hipSuccess && src->d_filter) {
        const uint64_t fbytes = 8ull << src->filter_log2_words;
        e = hipMalloc(&img->d_filter, fbytes);
        if (e == hipSuccess)
            e = hipMemcpyPeer(img->d_filter, device, src->d_filter, src->device, fbytes);
        if (e == hipSuccess)
            img->filter_log2_words = src->filter_log2_words;
    }
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(KGX_EDEVICE, std::string("replicate: ") + hipGetErrorString(e));
    }
    /* the line index is the caller's choice per replica (kgx_image_set_line_index):
     * it doubles the HBM an image takes, and a device may already hold one */
    *out = img;
    return KGX_OK;
}

int kgx_image_from_memory(const void *file_bytes, uint64_t nbytes, int device, kgx_image **out)
{
    if (!file_bytes || !out || nbytes < sizeof(kgx_image_header))
        return fail(KGX_EINVAL, "bad image buffer");
    kgx_image_header h;
    std::memcpy(&h, file_bytes, sizeof(h));
    int rc = validate_header(h, nbytes);
    if (rc)
        return rc;
    kgx_image *img = nullptr;
    rc = image_alloc(device, h.num_sigs, &img);
    if (rc)
        return rc;
    hipError_t e = hipMemcpy(img->d_table, static_cast<const char *>(file_bytes) + sizeof(h),
                             h.num_sigs * sizeof(kgx_sig_kmer), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(KGX_EDEVICE, std::string("image upload: ") + hipGetErrorString(e));
    }
    return image_settle(img, out);
}

int kgx_image_build_synthetic(uint64_t n_keys, uint64_t num_sigs, int device, kgx_image **out,
                              uint64_t *n_stored)
{
    if (2 * n_keys >= num_sigs)
        return fail(KGX_EFULL, "Your Kmer hash is half-full (kguts.cc:213-216)");
    kgx_image *img = nullptr;
    int rc = image_alloc(device, num_sigs, &img);
    if (rc)
        return rc;
    unsigned long long *d_count = nullptr;
    if (hipMalloc(&d_count, sizeof(*d_count)) != hipSuccess) {
        kgx_image_close(img);
        return fail(KGX_ENOMEM, "counter allocation failed");
    }
    hipError_t e = launch_synth_image(img->d_table, num_sigs, n_keys, n_keys, true, d_count, nullptr);
    unsigned long long cnt = 0;
    if (e == hipSuccess)
        e = hipMemcpy(&cnt, d_count, sizeof(cnt), hipMemcpyDeviceToHost);
    (void)hipFree(d_count);
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(KGX_EDEVICE, std::string("synthetic build: ") + hipGetErrorString(e));
    }
    if (n_stored)
        *n_stored = cnt;
    return image_settle(img, out);
}

int kgx_image_build_synthetic_distinct(uint64_t n_keys, uint64_t n_distinct, uint64_t num_sigs, int device,
                                       kgx_image **out, uint64_t *n_entries)
{
    if (!out)
        return fail(KGX_EINVAL, "null output");
    /* the stream is searched up to 1/8 past n_distinct (a synthetic 8-mer
     * stream repeats keys ~2% of the time at 1e9 of 20^8); owners are 32-bit */
    const uint64_t upper = n_distinct + n_distinct / 8 + 1024;
    if (2 * upper >= num_sigs || upper >= (1ull << 32))
        return fail(KGX_EFULL, "Your Kmer hash is half-full (kguts.cc:213-216)");
    kgx_image *img = nullptr;
    int rc = image_alloc(device, num_sigs, &img);
    if (rc)
        return rc;
    DevBuf d_count, d_hist;
    hipError_t e = d_count.reserve(sizeof(unsigned long long));
    if (e == hipSuccess)
        e = d_hist.reserve(256 * sizeof(unsigned long long));
    unsigned long long cnt = 0;
    if (e == hipSuccess)
        e = launch_synth_image(img->d_table, num_sigs, n_keys, upper, false, d_count.as<unsigned long long>(),
                               nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&cnt, d_count.p, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e == hipSuccess && cnt < n_distinct) {
        kgx_image_close(img);
        return fail(KGX_ERANGE, "the synthetic stream holds fewer distinct keys than asked for");
    }
    /* radix select of the n_distinct-th smallest owner, a byte per pass */
    uint32_t prefix = 0, mask = 0;
    uint64_t k = n_distinct; /* 1-based rank within the current prefix */
    for (int shift = 24; e == hipSuccess && shift >= 0; shift -= 8) {
        unsigned long long h[256];
        e = launch_owner_hist(img->d_table, num_sigs, prefix, mask, (uint32_t)shift,
                              d_hist.as<unsigned long long>(), nullptr);
        if (e == hipSuccess)
            e = hipMemcpy(h, d_hist.p, sizeof(h), hipMemcpyDeviceToHost);
        if (e != hipSuccess)
            break;
        uint32_t b = 0;
        while (b < 255 && k > h[b])
            k -= h[b++];
        prefix |= b << shift;
        mask |= 255u << shift;
    }
    const uint64_t m = (uint64_t)prefix + 1; /* entries [0, m) hold exactly n_distinct keys */
    if (e == hipSuccess)
        e = launch_synth_image(img->d_table, num_sigs, n_keys, m, true, d_count.as<unsigned long long>(), nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&cnt, d_count.p, sizeof(cnt), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(KGX_EDEVICE, std::string("synthetic build: ") + hipGetErrorString(e));
    }
    if (cnt != n_distinct) {
        kgx_image_close(img);
        return fail(KGX_EDEVICE, "synthetic build stored " + std::to_string(cnt) + " keys, not " +
                                     std::to_string(n_distinct));
    }
    if (n_entries)
        *n_entries = m;
    return image_settle(img, out);
}

int kgx_image_build(const uint64_t *keys, const int32_t *function_index, const int32_t *otu_index,
                    const uint16_t *avg_from_end, const float *function_wt, uint64_t n, uint64_t num_sigs,
                    int device, kgx_image **out, uint64_t *n_stored)
{
    if (!out || (n && (!keys || !function_index || !otu_index || !avg_from_end || !function_wt)))
        return fail(KGX_EINVAL, "null argument");
    /* kguts.cc:209-213: every valid key counts (duplicates too) */
    uint64_t valid = 0;
    for (uint64_t i = 0; i < n; i++)
        valid += keys[i] <= MAX_ENCODED;
    if (valid >= num_sigs / 2)
        return fail(KGX_EFULL, "Your Kmer hash is half-full (kguts.cc:209-213)");
    kgx_image *img = nullptr;
    int rc = image_alloc(device, num_sigs, &img);
    if (rc)
        return rc;
    DevBuf d_keys, d_fi, d_otu, d_avg, d_wt, d_count;
    hipError_t e = hipSuccess;
    for (auto rq : {d_keys.reserve(std::max<uint64_t>(n, 1) * 8), d_fi.reserve(std::max<uint64_t>(n, 1) * 4),
                    d_otu.reserve(std::max<uint64_t>(n, 1) * 4), d_avg.reserve(std::max<uint64_t>(n, 1) * 2),
                    d_wt.reserve(std::max<uint64_t>(n, 1) * 4), d_count.reserve(8)})
        if (rq != hipSuccess)
            e = rq;
    if (e == hipSuccess && n) {
        e = hipMemcpy(d_keys.p, keys, n * 8, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d_fi.p, function_index, n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d_otu.p, otu_index, n * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d_avg.p, avg_from_end, n * 2, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(d_wt.p, function_wt, n * 4, hipMemcpyHostToDevice);
    }
    unsigned long long cnt = 0;
    if (e == hipSuccess)
        e = launch_entries_image(img->d_table, num_sigs, d_keys.as<uint64_t>(), d_fi.as<int32_t>(),
                                 d_otu.as<int32_t>(), d_avg.as<uint16_t>(), d_wt.as<float>(), n,
                                 d_count.as<unsigned long long>(), nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&cnt, d_count.p, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(e == hipErrorOutOfMemory ? KGX_ENOMEM : KGX_EDEVICE,
                    std::string("image build: ") + hipGetErrorString(e));
    }
    if (n_stored)
        *n_stored = cnt;
    return image_settle(img, out);
}

int kgx_image_close(kgx_image *img)
{
    if (!img)
        return KGX_OK;
    svc_shutdown(img);
    (void)hipSetDevice(img->device);
    if (img->d_table)
        (void)hipFree(img->d_table);
    if (img->d_packed)
        (void)hipFree(img->d_packed);
    drop_line_index(img);
    if (img->d_filter)
        (void)hipFree(img->d_filter);
    if (img->probe_stream) {
        (void)hipStreamSynchronize(img->probe_stream);
        (void)hipStreamDestroy(img->probe_stream);
    }
    delete img;
    return KGX_OK;
}

uint64_t kgx_image_num_sigs(const kgx_image *img) { return img ? img->num_sigs : 0; }
int kgx_image_device(const kgx_image *img) { return img ? img->device : -1; }
const void *kgx_image_table(const kgx_image *img) { return img ? img->d_table : nullptr; }
int kgx_image_layout(const kgx_image *img) { return img ? img->layout : -1; }

int kgx_image_set_filter(kgx_image *img, int log2_bits)
{
    if (!img || log2_bits < 0 || (log2_bits && (log2_bits < 12 || log2_bits > 40)))
        return fail(KGX_EINVAL, "filter size: 0 (none) or 2^12 .. 2^40 bits");
    /* the device-wide synchronisation below would wait out its instances,
     * and the filter buffer is replaced under any service a call starts */
    const auto hold = svc_shutdown_hold(img);
    HIP_TRY(hipSetDevice(img->device));
    HIP_TRY(hipDeviceSynchronize());
    if (img->d_filter)
        (void)hipFree(img->d_filter);
    img->d_filter = nullptr;
    img->filter_log2_words = 0;
    if (!log2_bits)
        return KGX_OK;
    const uint32_t lw = (uint32_t)log2_bits - 6;
    const uint64_t bytes = 8ull << lw;
    if (hipMalloc(&img->d_filter, bytes) != hipSuccess) {
        (void)hipGetLastError();
        img->d_filter = nullptr;
        return fail(KGX_ENOMEM, "no room for the filter");
    }
    HIP_TRY(hipMemset(img->d_filter, 0, bytes));
    HIP_TRY(launch_filter_build(img->resident(), img->layout, img->num_sigs, img->d_filter, lw, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    img->filter_log2_words = lw;
    return KGX_OK;
}

int kgx_image_set_layout(kgx_image *img, int layout)
{
    if (!img)
        return fail(KGX_EINVAL, "null image");
    /* its workgroups hold the resident table's address: no call starts a
     * service until the table it would use is the new one */
    const auto hold = svc_shutdown_hold(img);
    if (layout == KGX_LAYOUT_PACKED16)
        return image_pack(img);
    if (layout == KGX_LAYOUT_AOS24) {
        if (img->lines) { /* the line index holds PACKED16 records */
            HIP_TRY(hipSetDevice(img->device));
            HIP_TRY(hipDeviceSynchronize());
            drop_line_index(img);
        }
        return image_unpack(img);
    }
    return fail(KGX_EINVAL, "unknown layout " + std::to_string(layout));
}

/* buckets [first, first + count) in the file's format into host memory */
static int image_read(const kgx_image *img, uint64_t first, uint64_t count, kgx_sig_kmer *dst)
{
    HIP_TRY(hipSetDevice(img->device));
    if (img->layout == KGX_LAYOUT_AOS24) {
        HIP_TRY(hipMemcpy(dst, img->d_table + first, count * sizeof(kgx_sig_kmer), hipMemcpyDeviceToHost));
        return KGX_OK;
    }
    /* PACKED16: unpack slices on the device, then copy them out */
    const uint64_t slice = 1ull << 24; /* buckets (384 MiB of output) */
    kgx_sig_kmer *tmp = nullptr;
    HIP_TRY(hipMalloc(&tmp, std::max<uint64_t>(1, std::min(slice, count)) * sizeof(kgx_sig_kmer)));
    hipError_t e = hipSuccess;
    for (uint64_t b = 0; b < count && e == hipSuccess; b += slice) {
        const uint64_t m = std::min(slice, count - b);
        e = launch_unpack(img->d_packed + first + b, tmp, m, nullptr);
        if (e == hipSuccess)
            e = hipMemcpy(dst + b, tmp, m * sizeof(kgx_sig_kmer), hipMemcpyDeviceToHost);
    }
    (void)hipFree(tmp);
    if (e != hipSuccess)
        return fail(KGX_EDEVICE, std::string("download: ") + hipGetErrorString(e));
    return KGX_OK;
}

int kgx_image_download(const kgx_image *img, void *dst, uint64_t nbytes)
{
    if (!img || !dst || nbytes != img->num_sigs * sizeof(kgx_sig_kmer))
        return fail(KGX_EINVAL, "bad download buffer");
    return image_read(img, 0, img->num_sigs, static_cast<kgx_sig_kmer *>(dst));
}

int kgx_image_save(const kgx_image *img, const char *dir)
{
    if (!img || !dir)
        return fail(KGX_EINVAL, "null argument");
    const std::string path = std::string(dir) + "/kmer.table.mem_map";
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f)
        return fail(KGX_EIO, "could not open " + path + " for writing: " + std::strerror(errno));
    const kgx_image_header h{img->num_sigs, sizeof(kgx_sig_kmer), 1};
    bool ok = std::fwrite(&h, sizeof(h), 1, f) == 1;
    const uint64_t chunk = 1ull << 25; /* buckets per write (768 MiB) */
    std::vector<kgx_sig_kmer> buf(std::min(chunk, std::max<uint64_t>(img->num_sigs, 1)));
    for (uint64_t b = 0; ok && b < img->num_sigs; b += chunk) {
        const uint64_t m = std::min(chunk, img->num_sigs - b);
        int rc = image_read(img, b, m, buf.data());
        if (rc) {
            std::fclose(f);
            return rc;
        }
        ok = std::fwrite(buf.data(), sizeof(kgx_sig_kmer), m, f) == m;
    }
    if (std::fclose(f) != 0)
        ok = false;
    return ok ? KGX_OK : fail(KGX_EIO, "short write to " + path);
}

/* ---- contexts ------------------------------------------------------------ */

int kgx_ctx_create(kgx_image *img, kgx_ctx **out)
{
    if (!img || !out)
        return fail(KGX_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(img->device));
    /* KGX_PROBE_DEFER: the form of the line probe's aligned body for this
     * context (kgx_probe.hip): 1 or unset, a tile's chains past their first
     * line run once, packed, after every slice's first round; 0, each slice
     * runs its own rounds.  An A/B switch, read here like KGX_SMALL_BATCH */
    bool probe_defer = true;
    if (int rc = env_switch("KGX_PROBE_DEFER", "rounds per slice", "deferred", probe_defer))
        return rc;
    /* KGX_GUNZIP_DEVICE=0|1: the default of option "gunzip_device" for new
     * contexts (the handlers' own contexts have no other switch) */
    int64_t gunzip_device = CtxOptions{}.gunzip_device;
    if (const char *g = std::getenv("KGX_GUNZIP_DEVICE")) {
        if (*g && std::strcmp(g, "0") && std::strcmp(g, "1"))
            return fail(KGX_EINVAL, std::string("KGX_GUNZIP_DEVICE: 0 (host threads) or 1 (device), not \"") + g + "\"");
        if (*g)
            gunzip_device = *g == '1';
    }
    /* KGX_SCORE_LEAN=0|1|2: the default of option "score_lean" for new
     * contexts (alternated-process A/Bs) */
    int64_t score_lean = CtxOptions{}.score_lean;
    if (const char *l = std::getenv("KGX_SCORE_LEAN")) {
        if (*l && std::strcmp(l, "0") && std::strcmp(l, "1") && std::strcmp(l, "2"))
            return fail(KGX_EINVAL, std::string("KGX_SCORE_LEAN: 0 (general lane scorer), 1 (lean) or 2 (lean, "
                                                "packed), not \"") + l + "\"");
        if (*l)
            score_lean = *l - '0';
    }
    /* KGX_FQ_PARSE_DEVICE=0|1: the default of option "fq_parse_device" for
     * new contexts (the command line's own context has no other switch) */
    int64_t fq_parse_device = CtxOptions{}.fq_parse_device;
    if (const char *p = std::getenv("KGX_FQ_PARSE_DEVICE")) {
        if (*p && std::strcmp(p, "0") && std::strcmp(p, "1"))
            return fail(KGX_EINVAL, std::string("KGX_FQ_PARSE_DEVICE: 0 (host parser) or 1 (device), not \"") + p + "\"");
        if (*p)
            fq_parse_device = *p == '1';
    }
    /* KGX_FQ_BODY_DEVICE=0|1: the default of option "fq_body_device" for new
     * contexts (kgx_query and kgx_server reach their handlers' contexts so) */
    int64_t fq_body_device = CtxOptions{}.fq_body_device;
    if (const char *p = std::getenv("KGX_FQ_BODY_DEVICE")) {
        if (*p && std::strcmp(p, "0") && std::strcmp(p, "1"))
            return fail(KGX_EINVAL, std::string("KGX_FQ_BODY_DEVICE: 0 (host threads) or 1 (device), not \"") + p + "\"");
        if (*p)
            fq_body_device = *p == '1';
    }
    kgx_ctx *c = new kgx_ctx;
    c->img = img;
    c->probe_defer = probe_defer;
    c->opt.gunzip_device = gunzip_device;
    c->opt.score_lean = score_lean;
    c->opt.fq_parse_device = fq_parse_device;
    c->opt.fq_body_device = fq_body_device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(KGX_EDEVICE, std::string("stream: ") + hipGetErrorString(e));
    }
    c->own_stream = true;
    /* KGX_SMALL_BATCH: the default of option "small_batch" for new contexts */
    if (const char *sb = std::getenv("KGX_SMALL_BATCH"))
        c->opt.small_batch = std::min<int64_t>(1 << 24, std::max<int64_t>(0, std::atoll(sb)));
    e = hipEventCreateWithFlags(&c->probe_done, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(KGX_EDEVICE, std::string("event: ") + hipGetErrorString(e));
    }
    *out = c;
    return KGX_OK;
}

int kgx_ctx_destroy(kgx_ctx *c)
{
    if (!c)
        return KGX_OK;
    (void)hipSetDevice(c->img->device);
    if (c->twin)
        kgx_ctx_destroy(c->twin);
    (void)hipStreamSynchronize(c->stream);
    for (DevBuf *b : {&c->residues, &c->offsets, &c->wbase, &c->tile_seq, &c->hit_mask,
                      &c->hits, &c->calls, &c->hit_count, &c->call_count, &c->dense_hoff,
                      &c->dense_coff, &c->dense_hits, &c->dense_calls, &c->plan_ws, &c->ranges})
        b->release();
    {
        std::lock_guard<std::mutex> lock(c->img->probe_mu);
        if (c->img->last_probe == c->probe_done)
            c->img->last_probe = nullptr;
    }
    (void)hipEventDestroy(c->probe_done);
    if (c->probe_ready)
        (void)hipEventDestroy(c->probe_ready);
    if (c->score_gate)
        (void)hipEventDestroy(c->score_gate);
    c->pool.reset();
    c->stage_pool.reset();
    for (hipEvent_t e : c->chunk_done)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->chunk_counts)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->chunk_gathered)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->chunk_h2d)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->prof_ev)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->prof_done)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->gz_events)
        (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ft_events)
        (void)hipEventDestroy(e);
    if (c->copy_stream) {
        (void)hipStreamSynchronize(c->copy_stream);
        (void)hipStreamDestroy(c->copy_stream);
    }
    if (c->up_stream) {
        (void)hipStreamSynchronize(c->up_stream);
        (void)hipStreamDestroy(c->up_stream);
    }
    if (c->own_stream)
        (void)hipStreamDestroy(c->stream);
    delete c;
    return KGX_OK;
}

void *kgx_ctx_stream(kgx_ctx *c) { return c ? (void *)c->stream : nullptr; }

int kgx_ctx_set_stream(kgx_ctx *c, void *stream)
{
    if (!c)
        return fail(KGX_EINVAL, "null ctx");
    if (stream) {
        if (c->own_stream)
            (void)hipStreamDestroy(c->stream);
        c->stream = (hipStream_t)stream;
        c->own_stream = false;
    } else if (!c->own_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    return KGX_OK;
}

int kgx_ctx_set_option(kgx_ctx *c, const char *name, int64_t value)
{
    if (!c || !name)
        return fail(KGX_EINVAL, "null argument");
    std::string err;
    if (ctx_option_set(c->opt, name, value, &err))
        return fail(KGX_EINVAL, err);
    return KGX_OK;
}

int kgx_ctx_get_option(kgx_ctx *c, const char *name, int64_t *value)
{
    if (!c || !name || !value)
        return fail(KGX_EINVAL, "null argument");
    if (!ctx_option_get(c->opt, name, value))
        return fail(KGX_EINVAL, std::string("unknown option ") + name);
    return KGX_OK;
}

int kgx_ctx_memcpy_d2d(kgx_ctx *c, void *dst, const void *src, uint64_t n)
{
    if (!c || (n && (!dst || !src)))
        return fail(KGX_EINVAL, "null argument");
    if (n)
        HIP_TRY(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream));
    return KGX_OK;
}

int kgx_ctx_check(kgx_ctx *c)
{
    if (!c)
        return fail(KGX_EINVAL, "null ctx");
    HIP_TRY(hipSetDevice(c->img->device));
    if (!c->plan_status.p)
        return KGX_OK; /* nothing planned yet */
    HIP_TRY(c->h_plan_status.resize(1));
    HIP_TRY(hipMemcpyAsync(c->h_plan_status.data(), c->plan_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->h_plan_status[0])
        return fail(KGX_EINVAL, "batch offsets not monotone or spanning more than n_residues bytes "
                                "(the batch was processed as empty)");
    return KGX_OK;
}

int kgx_ctx_synchronize(kgx_ctx *c)
{
    if (!c)
        return fail(KGX_EINVAL, "null ctx");
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KGX_OK;
}

/* ---- stages ------------------------------------------------------------- */

int kgx_stage_plan(kgx_ctx *c, const uint64_t *d_off, uint32_t n_seq, uint64_t n_residues)
{
    if (!c || (!d_off && n_seq))
        return fail(KGX_EINVAL, "null argument");
    if (n_residues > (1ull << 40))
        return fail(KGX_ERANGE, "batch too large");
    HIP_TRY(hipSetDevice(c->img->device));
    int rc = kgx::plan_reserve(c, d_off, n_seq, n_residues);
    if (rc)
        return rc;
    if (c->opt.plan_fused == 2 && n_seq <= (1u << 18)) {
        HIP_TRY(launch_plan_one(d_off, n_seq, n_residues, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(),
                                c->tile_windows, c->max_tiles, c->plan_status.as<uint32_t>(), c->stream));
        return KGX_OK;
    }
    if (c->opt.plan_fused == 1) {
        /* new states start at zero (every launch leaves them so); a grown
         * buffer may come back at the old address, so its capacity says */
        const size_t had = c->plan_look.cap;
        HIP_TRY(c->plan_look.reserve(plan_look_bytes(n_seq)));
        if (c->plan_look.cap != had)
            HIP_TRY(hipMemsetAsync(c->plan_look.p, 0, c->plan_look.cap, c->stream));
        HIP_TRY(launch_plan_fused(d_off, n_seq, n_residues, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(),
                                  c->tile_windows, c->max_tiles, c->plan_look.p, c->plan_status.as<uint32_t>(),
                                  c->stream));
        return KGX_OK;
    }
    HIP_TRY(c->plan_ws.reserve(plan_workspace_bytes(n_seq)));
    HIP_TRY(launch_plan(d_off, n_seq, n_residues, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(),
                        c->tile_windows, c->plan_ws.p, c->plan_status.as<uint32_t>(), c->stream));
    return KGX_OK;
}

}  // extern "C"

namespace kgx {

/* the plan's buffers and bookkeeping (everything of kgx_stage_plan but the
 * plan kernels; the small-batch path writes the plan from the host) */
int plan_reserve(kgx_ctx *c, const uint64_t *d_off, uint32_t n_seq, uint64_t n_residues)
{
    /* bounds: windows <= residues, so tiles <= residues / tile + 1 */
    const uint32_t tile_windows = 64u * (uint32_t)c->opt.probe_j;
    const uint64_t max_tiles = n_residues / tile_windows + 1;
    const uint64_t cap_win = std::max<uint64_t>(n_residues, 1);
    HIP_TRY(c->wbase.reserve((n_seq + 1) * sizeof(uint64_t)));
    HIP_TRY(c->tile_seq.reserve(max_tiles * sizeof(uint32_t)));
    HIP_TRY(c->hit_mask.reserve((cap_win / 64 + 2) * sizeof(uint64_t)));
    /* HIT_PACKED16: one 16-B record per slot; HIT_PLANES: hot plane, then cold plane */
    const bool packed_hits = c->img->layout == KGX_LAYOUT_PACKED16;
    HIP_TRY(c->hits.reserve(cap_win * (packed_hits ? 1 : 2) * sizeof(uint4)));
    HIP_TRY(c->calls.reserve(cap_win * sizeof(kgx_call)));
    HIP_TRY(c->ranges.reserve(cap_win * 2 * sizeof(uint32_t)));
    HIP_TRY(c->hit_count.reserve((n_seq + 1) * sizeof(uint32_t)));
    HIP_TRY(c->call_count.reserve((n_seq + 1) * sizeof(uint32_t)));
    HIP_TRY(c->plan_status.reserve(4 * sizeof(uint32_t))); /* [0] bad offsets, [1] longest sequence (windows) */
    c->n_seq = n_seq;
    c->n_residues = n_residues;
    c->max_tiles = max_tiles;
    c->tile_windows = tile_windows;
    c->hit_slots = cap_win;
    c->d_off = d_off;
    c->counts_enqueued = 0;
    c->have_hits = false;
    c->have_best = false;
    c->have_otus = false;
    return KGX_OK;
}

}  // namespace kgx

namespace {

/* option probe_persist: the line probe's grid capped at that many
 * workgroups per CU (0 = uncapped) */
uint32_t probe_max_blocks(const kgx_ctx *c)
{
    if (!c->opt.probe_persist)
        return 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->img->device) != hipSuccess || cus <= 0)
        cus = 256;
    return (uint32_t)c->opt.probe_persist * (uint32_t)cus;
}

/* what a probe launcher takes beside ctx_probe_table(c): c's planned batch
 * over `bytes` (residues with offsets, or bases with anchors), its hit
 * buffers, its options */
struct CtxProbe {
    ProbeBatch batch;
    ProbeHits hits;
    ProbeRun run;
};
CtxProbe ctx_probe(kgx_ctx *c, const uint8_t *bytes, uint64_t n_bytes, const uint64_t *starts)
{
    CtxProbe p;
    p.batch = {bytes, n_bytes, starts, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(), c->n_seq, c->max_tiles};
    p.hits = {c->hits.as<uint4>(), c->hits.as<uint4>() + c->hit_slots, c->hit_mask.as<uint64_t>()};
    p.run = {(int)(c->tile_windows / 64), (int)c->opt.probe_variant, (uint32_t)c->opt.probe_lds_kb, probe_max_blocks(c),
             c->probe_defer, (uint32_t)c->opt.probe_nt};
    return p;
}

/* one probe launch on c's stream; with probe_serialize it waits for the
 * image's previous probe, whichever context issued it */
template <class Launch>
int probe_chained(kgx_ctx *c, Launch launch)
{
    HIP_TRY(hipSetDevice(c->img->device));
    if (c->img->num_sigs >= (1ull << 40))
        return fail(KGX_ERANGE, "image too large");
    kgx_image *img = c->img;
    std::unique_lock<std::mutex> lock(img->probe_mu, std::defer_lock);
    if (c->opt.probe_serialize && c->opt.probe_stream) {
        /* option probe_stream: every chained probe of the image on one stream
         * (one hardware queue), entered when this context's inputs are ready
         * and left back to this context's stream */
        lock.lock();
        if (!img->probe_stream)
            HIP_TRY(hipStreamCreateWithFlags(&img->probe_stream, hipStreamNonBlocking));
        if (!c->probe_ready)
            HIP_TRY(hipEventCreateWithFlags(&c->probe_ready, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->probe_ready, c->stream));
        HIP_TRY(hipStreamWaitEvent(img->probe_stream, c->probe_ready, 0));
        hipStream_t own = c->stream;
        c->stream = img->probe_stream; /* the launch reads c->stream */
        const hipError_t le = launch();
        c->stream = own;
        HIP_TRY(le);
        HIP_TRY(hipEventRecord(c->probe_done, img->probe_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->probe_done, 0));
        img->last_probe = c->probe_done;
    } else {
        if (c->opt.probe_serialize) {
            lock.lock();
            if (img->last_probe && img->last_probe != c->probe_done)
                HIP_TRY(hipStreamWaitEvent(c->stream, img->last_probe, 0));
        }
        HIP_TRY(launch());
        if (c->opt.probe_serialize) {
            HIP_TRY(hipEventRecord(c->probe_done, c->stream));
            img->last_probe = c->probe_done;
        }
    }
    /* every PACKED16 probe stores the matching record itself */
    c->hit_format = c->img->layout == KGX_LAYOUT_PACKED16 ? HIT_PACKED16 : HIT_PLANES;
    c->have_hits = true;
    return KGX_OK;
}

}  // namespace

namespace kgx {

bool probe_takes_dna(const kgx_ctx *c)
{
    return c->img->layout == KGX_LAYOUT_PACKED16 && !(c->opt.probe_filter && c->img->d_filter) &&
           (c->opt.probe_variant == PROBE_AUTO || c->opt.probe_variant == PROBE_LINE) && c->opt.probe_j >= 1 && c->opt.probe_j <= 4;
}

int stage_probe_dna(kgx_ctx *c, const uint8_t *bases, uint64_t n_bases, const uint64_t *anchors,
                    const uint64_t *d_off)
{
    if ((!anchors || !bases) && c->n_seq)
        return fail(KGX_EINVAL, "fq probe: anchors or bases missing");
    if (d_off != c->d_off)
        return fail(KGX_EINVAL, "fq probe: offsets differ from the plan");
    if (!probe_takes_dna(c) || (int)(c->tile_windows / 64) != c->opt.probe_j)
        return fail(KGX_EINVAL, "fq probe: fragments without residues need the line probe on a PACKED16 image "
                                "(set fq_residues 1 for other probes)");
    return probe_chained(c, [&] {
        const CtxProbe p = ctx_probe(c, bases, n_bases, anchors);
        return launch_probe_dna(p.batch, ctx_probe_table(c), p.hits, p.run, c->stream);
    });
}

}  // namespace kgx

extern "C" {

int kgx_stage_probe(kgx_ctx *c, const uint8_t *d_res, const uint64_t *d_off)
{
    if (!c || (!d_res && c->n_residues) || d_off != c->d_off)
        return fail(KGX_EINVAL, "probe: residues missing or offsets differ from the plan");
    return probe_chained(c, [&] {
        const CtxProbe p = ctx_probe(c, d_res, c->n_residues, d_off);
        return launch_probe(p.batch, ctx_probe_table(c), p.hits, p.run, c->stream);
    });
}



int kgx_stage_score(kgx_ctx *c, const kgx_params *params, uint32_t want)
{
    if (!c)
        return fail(KGX_EINVAL, "null ctx");
    kgx_params p;
    if (params)
        p = *params;
    else
        kgx_params_default(&p);
    HIP_TRY(hipSetDevice(c->img->device));
    const bool best = (want & KGX_WANT_BEST) != 0;
    bool lean_taken = false;
    HIP_TRY(launch_score(c->n_seq, c->n_residues, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(), c->max_tiles,
                         c->hit_mask.as<uint64_t>(), c->tile_windows, c->hits.as<uint4>(), c->calls.as<kgx_call>(),
                         c->ranges.p, c->hit_count.as<uint32_t>(), c->call_count.as<uint32_t>(), p,
                         want | (best ? KGX_WANT_CALLS : 0u), c->hit_format, c->opt.score_variant,
                         (uint32_t)c->opt.score_wave_tiles, (int)c->opt.score_lean, c->plan_status.as<uint32_t>(),
                         c->stream, &lean_taken));
    c->lean_scores += lean_taken;
    c->have_best = false;
    c->have_otus = false;
    if (want & KGX_WANT_OTU) {
        HIP_TRY(c->otu_ws.reserve(std::max<uint64_t>(c->hit_slots, 1) * sizeof(int32_t)));
        HIP_TRY(c->otus.reserve(std::max<uint64_t>(c->hit_slots, 1) * sizeof(kgx_otu)));
        HIP_TRY(c->otu_count.reserve(std::max<uint64_t>(c->n_seq, 1) * sizeof(uint32_t)));
        HIP_TRY(launch_otus(c->n_seq, c->wbase.as<uint64_t>(), c->hit_mask.as<uint64_t>(), c->tile_windows,
                            c->hits.as<uint4>(), c->hits.as<uint4>() + c->hit_slots, c->otu_ws.as<int32_t>(),
                            c->otus.as<kgx_otu>(), c->otu_count.as<uint32_t>(), c->hit_format, c->stream));
        c->have_otus = true;
    }
    if (best) {
        HIP_TRY(c->best.reserve(std::max<uint64_t>(c->n_seq, 1) * sizeof(kgx_best_call)));
        HIP_TRY(c->best_ws.reserve(c->hit_slots * sizeof(kgx_call)));
        if (!c->defer_best)
            HIP_TRY(launch_best_calls(c->n_seq, c->calls.as<kgx_call>(), c->wbase.as<uint64_t>(),
                                      c->call_count.as<uint32_t>(), c->best_ws.as<kgx_call>(),
                                      c->best.as<kgx_best_call>(), c->stream));
        c->have_best = true;
    }
    return KGX_OK;
}

int kgx_find_best_calls(kgx_ctx *c, const kgx_call *calls, const uint64_t *call_offsets, uint32_t n_seq,
                        kgx_best_call *out)
{
    if (!c || (n_seq && (!call_offsets || !out)))
        return fail(KGX_EINVAL, "null argument");
    if (n_seq == 0)
        return KGX_OK;
    const uint64_t c0 = call_offsets[0], n = call_offsets[n_seq] - c0;
    if (n && !calls)
        return fail(KGX_EINVAL, "null calls");
    std::vector<uint64_t> start(n_seq);
    std::vector<uint32_t> count(n_seq);
    for (uint32_t s = 0; s < n_seq; s++) {
        if (call_offsets[s + 1] < call_offsets[s])
            return fail(KGX_EINVAL, "call_offsets not monotone");
        start[s] = call_offsets[s] - c0;
        count[s] = (uint32_t)(call_offsets[s + 1] - call_offsets[s]);
    }
    HIP_TRY(hipSetDevice(c->img->device));
    HIP_TRY(c->bc_calls.reserve(std::max<uint64_t>(n, 1) * sizeof(kgx_call)));
    HIP_TRY(c->best_ws.reserve(std::max<uint64_t>(n, 1) * sizeof(kgx_call)));
    HIP_TRY(c->bc_start.reserve(n_seq * sizeof(uint64_t)));
    HIP_TRY(c->bc_count.reserve(n_seq * sizeof(uint32_t)));
    HIP_TRY(c->best.reserve(n_seq * sizeof(kgx_best_call)));
    c->have_best = false; /* best[] now belongs to this call, not to the plan */
    if (n)
        HIP_TRY(hipMemcpyAsync(c->bc_calls.p, calls + c0, n * sizeof(kgx_call), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bc_start.p, start.data(), n_seq * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->bc_count.p, count.data(), n_seq * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_best_calls(n_seq, c->bc_calls.as<kgx_call>(), c->bc_start.as<uint64_t>(),
                              c->bc_count.as<uint32_t>(), c->best_ws.as<kgx_call>(), c->best.as<kgx_best_call>(),
                              c->stream));
    HIP_TRY(hipMemcpyAsync(out, c->best.p, n_seq * sizeof(kgx_best_call), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return KGX_OK;
}

int kgx_device_result_get(kgx_ctx *c, kgx_device_result *out)
{
    if (!c || !out)
        return fail(KGX_EINVAL, "null argument");
    out->n_seq = c->n_seq;
    out->tile_windows = c->tile_windows;
    out->window_base = c->wbase.as<uint64_t>();
    out->hit_mask = c->hit_mask.as<uint64_t>();
    out->hit_count = c->hit_count.as<uint32_t>();
    out->call_count = c->call_count.as<uint32_t>();
    out->hits_hot = c->hits.as<uint32_t>();
    out->hits_cold = c->hit_format == HIT_PLANES ? c->hits.as<uint32_t>() + 4 * c->hit_slots : nullptr;
    out->hit_format = c->hit_format;
    out->otu_count = c->have_otus ? c->otu_count.as<uint32_t>() : nullptr;
    out->otus = c->have_otus ? c->otus.as<kgx_otu>() : nullptr;
    out->calls = c->calls.as<kgx_call>();
    out->best = c->have_best ? c->best.as<kgx_best_call>() : nullptr;
    return KGX_OK;
}

int kgx_run_device(kgx_ctx *c, const kgx_params *params, const uint8_t *d_res, const uint64_t *d_off,
                   uint32_t n_seq, uint64_t n_residues, uint32_t want, kgx_device_result *out)
{
    int rc = kgx_stage_plan(c, d_off, n_seq, n_residues);
    if (rc)
        return rc;
    if ((rc = kgx_stage_probe(c, d_res, d_off)))
        return rc;
    if (c->score_stream) {
        /* the score on its own stream behind the probe (kgx_pool_lookup) */
        if (!c->score_gate)
            HIP_TRY(hipEventCreateWithFlags(&c->score_gate, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->score_gate, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->score_stream, c->score_gate, 0));
        hipStream_t own = c->stream;
        c->stream = c->score_stream;
        rc = kgx_stage_score(c, params, want);
        c->stream = own;
        if (rc)
            return rc;
    } else if ((rc = kgx_stage_score(c, params, want))) {
        return rc;
    }
    return out ? kgx_device_result_get(c, out) : KGX_OK;
}

int kgx_fq_run_device(kgx_ctx *c, const kgx_params *params, const kgx_fragments *fr, uint32_t want,
                      kgx_device_result *out)
{
    if (!c || !fr)
        return fail(KGX_EINVAL, "null argument");
    if (fr->residues || fr->n_fragments == 0)
        return kgx_run_device(c, params, fr->residues, fr->offsets, fr->n_fragments, fr->n_residues, want, out);
    /* the DNA probe's own tile (option fq_probe_j): its encode reads 24
     * bases and 32 table entries per window, and one slice per wave keeps
     * more waves' line requests in flight (C4 probe 4.0-4.3 vs 4.4-4.9 ms per
     * 1M reads at J = 1 vs 2, profiles/r3e_fq_probe_j_sweep.json).  The plan,
     * probe and score of the pass use it; the result carries its tile size. */
    HIP_TRY(hipSetDevice(c->img->device));
    const int keep_j = c->opt.probe_j;
    if (c->opt.fq_probe_j)
        c->opt.probe_j = c->opt.fq_probe_j;
    /* this context's own fragments (>= 11 residues each) are planned by one
     * elementwise kernel instead of launch_plan's reduce / scan / scan */
    const bool own = c->opt.fq_plan && fr->offsets == c->fq_off.as<uint64_t>();
    int rc = own ? kgx::plan_reserve(c, fr->offsets, fr->n_fragments, fr->n_residues)
                 : kgx_stage_plan(c, fr->offsets, fr->n_fragments, fr->n_residues);
    if (!rc && own) {
        /* one longest-fragment word per 256-fragment workgroup */
        hipError_t e = c->plan_ws.reserve(((size_t)fr->n_fragments / 256 + 2) * sizeof(uint32_t));
        if (e == hipSuccess)
            e = launch_fq_plan(fr->offsets, fr->n_fragments, c->wbase.as<uint64_t>(), c->tile_seq.as<uint32_t>(),
                               c->tile_windows, c->plan_status.as<uint32_t>(), c->plan_ws.as<uint32_t>(), c->stream);
        if (e != hipSuccess)
            rc = fail(KGX_EDEVICE, std::string("fq plan: ") + hipGetErrorString(e));
    }
    if (!rc)
        rc = stage_probe_dna(c, fr->bases, fr->n_bases, fr->anchors, fr->offsets);
    c->opt.probe_j = keep_j;
    if (rc)
        return rc;
    if ((rc = kgx_stage_score(c, params, want)))
        return rc;
    return out ? kgx_device_result_get(c, out) : KGX_OK;
}

}  // extern "C"

extern "C" {

int kgx_ctx_stat(kgx_ctx *c, const char *name, int64_t *value)
{
    if (!c || !name || !value)
        return fail(KGX_EINVAL, "null argument");
    const std::string n = name;
    if (n == "fused_batches")
        *value = (int64_t)c->fused_batches;
    else if (n == "small_batches")
        *value = (int64_t)c->small_batches;
    else if (n == "stream_fallbacks")
        *value = (int64_t)c->stream_fallbacks;
    else if (n == "pinned_batches")
        *value = (int64_t)c->pinned_batches;
    else if (n == "nul_reruns")
        *value = (int64_t)c->nul_reruns;
    else if (n == "lean_scores")
        *value = (int64_t)c->lean_scores;
    else if (n == "fq_parses")
        *value = (int64_t)c->fq_parses;
    else
        return fail(KGX_EINVAL, "unknown statistic " + n);
    return KGX_OK;
}

int kgx_ctx_host_profile(kgx_ctx *c, kgx_host_profile *out)
{
    if (!c || !out)
        return fail(KGX_EINVAL, "null argument");
    *out = c->last_profile;
    return KGX_OK;
}

/* the current device batch's results -> host CSR (gather on the device, OTU
 * tallies on the host) */
int kgx_device_batch_collect(kgx_ctx *c, uint32_t want, kgx_result *out)
{
    if (!c || !out)
        return fail(KGX_EINVAL, "null argument");
    if (!c->have_hits)
        return fail(KGX_EINVAL, "no device batch to collect");
    const bool want_calls = (want & KGX_WANT_CALLS) != 0;
    const bool want_otu = (want & KGX_WANT_OTU) != 0;
    const bool need_hits = (want & KGX_WANT_HITS) != 0;
    const bool want_best = (want & KGX_WANT_BEST) != 0;
    if (want_otu && !c->have_otus)
        return fail(KGX_EINVAL, "no device OTU tallies (score with KGX_WANT_OTU)");
    if (want_best && !c->have_best)
        return fail(KGX_EINVAL, "no device best calls (score with KGX_WANT_BEST)");
    HIP_TRY(hipSetDevice(c->img->device));
    PhaseTimer tm(c);
    const uint32_t n_seq = c->n_seq;
    /* counts -> dense CSR offsets on the host, gather on the device.  The
     * plan's status word (bad device offsets: an error, not an empty result)
     * and the window total come back with the counts, in one round trip
     * (collect_counts_enqueue, unless already enqueued). */
    const bool best_now = want_best && n_seq && !need_hits && !want_calls && !want_otu;
    if (c->counts_enqueued != want + 1) {
        if (int rc = kgx::collect_counts_enqueue(c, want))
            return rc;
    }
    c->counts_enqueued = 0;
    HIP_TRY(host_wait(c->stream));
    if (c->h_plan_status[0])
        return fail(KGX_EINVAL, "batch offsets not monotone or spanning more than n_residues bytes "
                                "(the batch was processed as empty)");
    c->h_hoff.assign(n_seq + 1, 0);
    c->h_coff.assign(n_seq + 1, 0);
    c->h_ooff.assign(n_seq + 1, 0);
    for (uint32_t s = 0; s < n_seq; s++) {
        c->h_hoff[s + 1] = c->h_hoff[s] + c->h_hcount[s];
        c->h_coff[s + 1] = c->h_coff[s] + (want_calls ? c->h_ccount[s] : 0);
        c->h_ooff[s + 1] = c->h_ooff[s] + (want_otu ? c->h_ocount[s] : 0);
    }
    tm.mark(" counts");
    const uint64_t nh = c->h_hoff[n_seq], nc = c->h_coff[n_seq], no = c->h_ooff[n_seq];
    HIP_TRY(c->h_hits.resize(need_hits ? nh : 0));
    HIP_TRY(c->h_calls.resize(nc));
    HIP_TRY(c->h_otus.resize(no));
    /* small results: the gather stores the records straight into the mapped
     * pinned result arrays (no D2H copies to queue behind it) */
    const bool mapped = (need_hits ? nh : 0) + nc + no <= (1u << 16);
    if ((need_hits && nh) || nc || no) {
        HIP_TRY(c->dense_hoff.reserve((n_seq + 1) * sizeof(uint64_t)));
        HIP_TRY(c->dense_coff.reserve((n_seq + 1) * sizeof(uint64_t)));
        HIP_TRY(c->dense_ooff.reserve((n_seq + 1) * sizeof(uint64_t)));
        HIP_TRY(c->dense_hits.reserve(std::max<uint64_t>(nh, 1) * sizeof(kgx_hit)));
        HIP_TRY(c->dense_calls.reserve(std::max<uint64_t>(nc, 1) * sizeof(kgx_call)));
        HIP_TRY(c->dense_otus.reserve(std::max<uint64_t>(no, 1) * sizeof(kgx_otu)));
        HIP_TRY(hipMemcpyAsync(c->dense_hoff.p, c->h_hoff.data(), (n_seq + 1) * sizeof(uint64_t),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dense_coff.p, c->h_coff.data(), (n_seq + 1) * sizeof(uint64_t),
                               hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->dense_ooff.p, c->h_ooff.data(), (n_seq + 1) * sizeof(uint64_t),
                               hipMemcpyHostToDevice, c->stream));
        void *mh = nullptr, *mc = nullptr, *mo = nullptr;
        if (mapped) {
            if (need_hits && nh)
                HIP_TRY(c->h_hits.device_ptr(0, &mh));
            if (nc)
                HIP_TRY(c->h_calls.device_ptr(0, &mc));
            if (no)
                HIP_TRY(c->h_otus.device_ptr(0, &mo));
        }
        kgx_hit *gh = need_hits && nh ? (mapped ? static_cast<kgx_hit *>(mh) : c->dense_hits.as<kgx_hit>()) : nullptr;
        kgx_call *gc = want_calls ? (mapped && nc ? static_cast<kgx_call *>(mc) : c->dense_calls.as<kgx_call>())
                                  : nullptr;
        kgx_otu *go = no ? (mapped ? static_cast<kgx_otu *>(mo) : c->dense_otus.as<kgx_otu>()) : nullptr;
        HIP_TRY(launch_gather(n_seq, c->wbase.as<uint64_t>(), c->hit_mask.as<uint64_t>(), c->tile_windows,
                              c->call_count.as<uint32_t>(), c->hits.as<uint4>(),
                              c->hits.as<uint4>() + c->hit_slots,
                              c->calls.as<kgx_call>(), c->dense_hoff.as<uint64_t>(),
                              c->dense_coff.as<uint64_t>(), gh, gc, 0u, c->hit_format,
                              c->otu_count.as<uint32_t>(), c->otus.as<kgx_otu>(), c->dense_ooff.as<uint64_t>(),
                              go, c->stream));
        if (!mapped) {
            if (need_hits && nh)
                HIP_TRY(hipMemcpyAsync(c->h_hits.data(), c->dense_hits.p, nh * sizeof(kgx_hit),
                                       hipMemcpyDeviceToHost, c->stream));
            if (nc)
                HIP_TRY(hipMemcpyAsync(c->h_calls.data(), c->dense_calls.p, nc * sizeof(kgx_call),
                                       hipMemcpyDeviceToHost, c->stream));
            if (no)
                HIP_TRY(hipMemcpyAsync(c->h_otus.data(), c->dense_otus.p, no * sizeof(kgx_otu),
                                       hipMemcpyDeviceToHost, c->stream));
        }
    }
    if (want_best && n_seq && !best_now) {
        HIP_TRY(c->h_best.resize(n_seq));
        HIP_TRY(hipMemcpyAsync(c->h_best.data(), c->best.p, n_seq * sizeof(kgx_best_call), hipMemcpyDeviceToHost,
                               c->stream));
    }
    if (!best_now)
        HIP_TRY(host_wait(c->stream));
    tm.mark(" gather+d2h");
    fill_result(c, n_seq, need_hits, want_best, c->h_nwin[0], out);
    return KGX_OK;
}

/* ---- synthetic queries / memory helpers ----------------------------------- */

int kgx_synth_queries(kgx_ctx *c, uint64_t image_n_keys, uint32_t n_seq, uint32_t length,
                      uint32_t x_permille, uint64_t q0, uint8_t *d_res, uint64_t *d_off)
{
    if (!c || !d_res || !d_off)
        return fail(KGX_EINVAL, "null argument");
    HIP_TRY(hipSetDevice(c->img->device));
    HIP_TRY(launch_synth_queries(image_n_keys, n_seq, length, x_permille, q0, d_res, d_off,
                                 c->stream));
    return KGX_OK;
}

int kgx_microbench_random_read(kgx_ctx *c, uint64_t n_reads, int mode, float *ms, uint64_t *reads)
{
    if (!c || !ms || mode < 0 || mode > 5)
        return fail(KGX_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->img->device));
    const uint64_t threads = 256ull * 256 * (uint64_t)c->opt.microbench_wgs; /* workgroups of 256 per CU */
    const int ilp = c->opt.microbench_ilp;
    const uint32_t rounds = (uint32_t)std::max<uint64_t>(1, n_reads / (threads * (uint64_t)ilp));
    HIP_TRY(c->plan_ws.reserve(threads * sizeof(uint64_t)));
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    HIP_TRY(hipEventRecord(a, c->stream));
    const uint64_t span = c->opt.microbench_span ? std::min((uint64_t)c->opt.microbench_span, c->img->resident_bytes())
                                             : c->img->resident_bytes();
    HIP_TRY(launch_random_read(c->img->resident(), span, threads, rounds, mode, ilp,
                               c->plan_ws.as<uint64_t>(), c->stream));
    HIP_TRY(hipEventRecord(b, c->stream));
    HIP_TRY(hipEventSynchronize(b));
    HIP_TRY(hipEventElapsedTime(ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (reads)
        *reads = threads * rounds * (uint64_t)ilp / (mode == 4 ? 4 : mode == 5 ? 8 : 1);
    return KGX_OK;
}

int kgx_event_create(void **event)
{
    if (!event)
        return fail(KGX_EINVAL, "null event");
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    *event = (void *)e;
    return KGX_OK;
}

int kgx_event_destroy(void *event)
{
    if (event)
        HIP_TRY(hipEventDestroy((hipEvent_t)event));
    return KGX_OK;
}

int kgx_event_record(void *event, kgx_ctx *c)
{
    if (!event || !c)
        return fail(KGX_EINVAL, "null argument");
    HIP_TRY(hipEventRecord((hipEvent_t)event, c->stream));
    return KGX_OK;
}

int kgx_event_elapsed_ms(void *start, void *end, float *ms)
{
    if (!start || !end || !ms)
        return fail(KGX_EINVAL, "null argument");
    HIP_TRY(hipEventSynchronize((hipEvent_t)end));
    HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)end));
    return KGX_OK;
}

int kgx_device_alloc(int device, uint64_t nbytes, void **out)
{
    if (!out)
        return fail(KGX_EINVAL, "null output");
    HIP_TRY(hipSetDevice(device));
    hipError_t e = hipMalloc(out, std::max<uint64_t>(nbytes, 1));
    if (e != hipSuccess)
        return fail(KGX_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return KGX_OK;
}

int kgx_device_free(void *p)
{
    if (p)
        HIP_TRY(hipFree(p));
    return KGX_OK;
}

int kgx_host_alloc(uint64_t nbytes, void **out)
{
    if (!out)
        return fail(KGX_EINVAL, "null output");
    *out = nullptr;
    /* portable: usable by every device's copies (the pool's replicas) */
    hipError_t e = hipHostMalloc(out, std::max<uint64_t>(nbytes, 1), hipHostMallocPortable);
    if (e != hipSuccess) {
        *out = nullptr;
        return fail(KGX_ENOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    return KGX_OK;
}

int kgx_host_free(void *p)
{
    if (p)
        HIP_TRY(hipHostFree(p));
    return KGX_OK;
}

int kgx_memcpy_h2d(void *dst, const void *src, uint64_t n)
{
    HIP_TRY(hipMemcpy(dst, src, n, hipMemcpyHostToDevice));
    return KGX_OK;
}

int kgx_memcpy_d2h(void *dst, const void *src, uint64_t n)
{
    HIP_TRY(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return KGX_OK;
}

}  /* extern "C" */

namespace kgx {

/* kgx_image_build's device half for entries already in HBM (kgx_sig.hip):
 * the same table allocation, insert and settling */
int image_from_device_entries(int device, uint64_t num_sigs, const uint64_t *d_keys, const int32_t *d_fi,
                              const int32_t *d_otu, const uint16_t *d_avg, const float *d_wt, uint64_t n,
                              kgx_image **out, uint64_t *n_stored)
{
    kgx_image *img = nullptr;
    int rc = image_alloc(device, num_sigs, &img);
    if (rc)
        return rc;
    DevBuf d_count;
    hipError_t e = d_count.reserve(8);
    unsigned long long cnt = 0;
    if (e == hipSuccess)
        e = launch_entries_image(img->d_table, num_sigs, d_keys, d_fi, d_otu, d_avg, d_wt, n,
                                 d_count.as<unsigned long long>(), nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&cnt, d_count.p, 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        kgx_image_close(img);
        return fail(e == hipErrorOutOfMemory ? KGX_ENOMEM : KGX_EDEVICE,
                    std::string("image build: ") + hipGetErrorString(e));
    }
    if (n_stored)
        *n_stored = cnt;
    return image_settle(img, out);
}

}  // namespace kgx
