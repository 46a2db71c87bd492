"""Benchmark of the hot path: protein residues/s against a 1B-entry k-mer image.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--n-keys 1e9] [--n-seq 100000]
        (N > 1 without torchrun: bench.py starts the N ranks itself, one per GPU)
        builds the image, warms up, times K steps and prints the result line
    python bench.py ... --dump-outputs DIR   the last timed step's results as DIR/<name>.npy
    python bench.py ... --full   also the canary, the kernel times and roofline, the parity
        check, the host-path / lookup / pool legs, the microbenchmark and the CPU baseline
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Workload (BASELINE.json configs[1], SURVEY §8(d) "C2"): per GPU, 100,000
synthetic 300-aa proteins (half planted copies of image proteins with 10%
substitutions, half uniform) against a synthetic 1B-entry signature image:
exactly 1,000,000,000 distinct keys (kgx_image_build_synthetic_distinct) in
the reference's 24-byte bucket format (num_sigs 3,559,786,523 by the builder's
sizing rule, 85.4 GB; alpha = 0.281), built directly in HBM.  Every rank holds
an image replica and its own query shard (weak scaling; no collective on the
data path -- torch.distributed is used for the barrier and the max-time
reduction).  --strong runs C5 instead (BASELINE.json configs[4]): one batch of
1,000,000 x 300 aa split across the ranks in residue-balanced shards
(shard.balanced_shards, the kgx_pool split), strong scaling.

A step = one pass over one resident batch: plan -> probe -> score
(kgx_run_device), inputs and outputs in HBM.  Steps rotate over --batches
distinct batches (so no step re-probes the lines the previous one left in
the 256 MiB Infinity Cache) and over --pipeline worker contexts (own stream +
buffers each, as the reference's thread pool keeps one KmerGuts per worker),
so one batch's scoring overlaps the next batch's probe.  The probe kernel is
timed with HIP events on the stream it runs on; the roofline uses SURVEY
§8(d)'s algorithmic bytes per window, (24 * P + 1), with P the mean buckets
examined per probed window measured by the CPU oracle on the rank-0 sample.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md chip table (spec)
METRIC = "protein residues/s vs 1B-entry kmer image; 1/2/4/8 MI355X"


def log(*a):
    print(*a, file=sys.stderr, flush=True)



def host_cpus():
    """(threads to use, CPUs in this process's affinity mask, cgroup CPU quota
    or None): SURVEY §8(d) d4's T = nproc, where a cgroup quota (cpu.max)
    caps what the affinity mask shows."""
    aff = len(os.sched_getaffinity(0))
    quota = None
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota = max(1, int(int(q) // int(period)))
    except (OSError, ValueError):
        quota = None
    return (min(aff, quota) if quota else aff), aff, quota


def cpu_baseline(oracle, table, res, off, threads, target_s, want):
    """The oracle (bit-exact CPU restatement) over a bounded sample of rank 0's
    batch (res/off: its first sequences, host copies of the device batch), on
    this host's cores, against a host copy of the same image.  The sample is
    processed repeatedly until about target_s seconds of timed work (the 85 GB
    table does not fit any CPU cache, so repeats still miss)."""
    secs, passes, probes, windows = 0.0, 0, 0, 0
    while secs < target_s and passes < 200:
        r = oracle.process_batch(table, res, off, want=want, n_threads=threads)
        secs += r.seconds
        passes += 1
        probes, windows = r.probes, r.windows
    r1 = oracle.process_batch(table, res, off, want=want, n_threads=1)
    cpu_model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    n_seq = len(off) - 1
    return {
        "cpu_model": cpu_model,
        "value": float(passes * len(res) / secs),
        "unit": "residues/s",
        "cores": threads,
        "kind": "port",
        "sample": f"{passes} passes over the first {n_seq} x {int(off[1] - off[0]) if n_seq else 0}-aa queries of "
                  f"rank 0's batch against a host copy of the same image ({WANT_NAMES.get(want, want)}, the GPU "
                  f"step's outputs), {threads} threads, {secs:.1f} s timed",
        "want": want,
        "single_thread_value": float(len(res) / r1.seconds),
        "pbar": probes / max(1, windows),
        "windows": int(windows),
    }


def parity_check(oracle, table, got, res, off, want, threads, line_index):
    """The timed configuration against the oracle over the whole batch: the
    device's results of rank 0's batch 0 (the timed want, the timed line
    index) and the oracle's over the same residues and image, every sequence,
    compared as bits (oracle.diff_batch: hits, calls, find_best_call)."""
    t0 = time.time()
    ref = oracle.process_batch(table, res, off, want=want, n_threads=threads)
    bad = oracle.diff_batch(got, ref, want)
    n_bad = sorted(set(i for v in bad.values() for i in v))
    out = {"sequences": len(off) - 1, "equal": not n_bad, "want": want,
           "outputs": sorted(bad), "line_index": line_index,
           "hits": int(ref.hit_offsets[-1]), "calls": int(ref.call_offsets[-1]),
           "differing_sequences": len(n_bad), "first_differing": n_bad[:8],
           "by_output": {k: len(v) for k, v in bad.items()},
           "check": "device results of batch 0 at the timed want and line index vs the CPU oracle over the "
                    "same 100% of sequences, compared as bits (oracle.diff_batch)",
           "seconds": round(time.time() - t0, 2)}
    return out, ref


WANT_NAMES = {3: "hits + calls", 7: "hits + calls + OTU", 11: "hits + calls + best call",
              15: "hits + calls + OTU + best call"}
# what each want mask is in the reference's handlers
WANT_OUTPUTS = {3: "hits + calls (lookup_request without find_best_match)",
                7: "hits + calls + OTU (add_request / query_request)",
                11: "hits + calls + device find_best_call per sequence (lookup_request find_best_match, "
                    "lookup_request.cc:166-210)",
                15: "hits + calls + OTU + device find_best_call"}


def canary_check(abi, synth, d, dev, line_index=0):
    """Every rank: the canary pass (close_kmers_amd/canary.py) on its own
    device, digested; the digests are gathered and compared with the CPU
    oracle's committed digest.  Returns (per-rank canary records, ok).  With
    more than one rank and no KGX_BENCH_DEVICE override, the ranks' devices
    must differ (one rank per GPU)."""
    from close_kmers_amd import canary
    t0 = time.time()
    mine = canary.run_on_device(abi, synth, dev, line_index)
    mine["rank"] = d.rank
    mine["seconds"] = round(time.time() - t0, 2)
    want = canary.expected()["digest"]
    mine["ok"] = mine["digest"] == want
    recs = d.gather_objects(mine)
    ok, why = canary.verdict(recs, want, d.world > 1 and "KGX_BENCH_DEVICE" not in os.environ)
    if not ok:
        log(f"[bench] canary: {why}")
    if d.rank == 0:
        log(f"[bench] canary ({canary.CANARY_SEQ} x {canary.CANARY_LEN} aa vs {canary.CANARY_KEYS:,}-entry image, "
            f"want {canary.CANARY_WANT}): " + ", ".join(
                f"rank {r['rank']} dev {r['device']} {'ok' if r['ok'] else 'MISMATCH ' + r['digest'][:16]}"
                for r in recs))
    return recs, ok


def pool_main(args) -> int:
    """--pool-devices N: the in-process multi-device serving shape (the
    reference's pool: one worker per execution resource over one image,
    threadpool.cc:18-44).  One process holds N replicas of the image (built on
    the first device, copied device to device by kgx_image_replicate onto
    device i % visible), runs BASELINE.json configs[4]'s batch (C5: 1M x
    300 aa, host buffers) through kgx_pool (residue-balanced shards, one
    context per replica, results concatenated in input order), checks the
    result byte for byte against one context's pass over the whole batch,
    and times the pool (compact results, as bench_pool).  Prints its own JSON
    line; exits non-zero on a mismatch."""
    from close_kmers_amd import abi, synth
    L = abi.lib()
    n_dev = abi.device_count()
    if n_dev < 1:
        raise SystemExit("no gfx950 device visible")
    N = args.pool_devices
    devices = [i % n_dev for i in range(N)]
    n_keys = int(args.n_keys)
    spec = synth.ImageSpec(n_keys, args.num_sigs or None)
    t0 = time.time()
    img0, _ = abi.Image.synthetic_distinct(spec.n_keys, n_keys, spec.num_sigs, device=devices[0])
    t_build = time.time() - t0
    t0 = time.time()
    images = [img0] + [img0.replicate(dv) for dv in devices[1:]]
    t_rep = time.time() - t0
    log(f"[pool] {n_keys:,}-key image on device {devices[0]} in {t_build:.1f}s, {N - 1} replica(s) on "
        f"{devices[1:]} in {t_rep:.1f}s")
    n, Ls = args.strong_seq, args.length
    ctx0 = abi.Context(img0)
    d_res, d_off = ctypes.c_void_p(), ctypes.c_void_p()
    abi.check(L.kgx_device_alloc(devices[0], n * Ls, ctypes.byref(d_res)), "alloc")
    abi.check(L.kgx_device_alloc(devices[0], (n + 1) * 8, ctypes.byref(d_off)), "alloc")
    abi.check(L.kgx_synth_queries(ctx0.handle, spec.n_keys, n, Ls, args.x_permille, 0, d_res, d_off), "queries")
    ctx0.synchronize()
    res = np.empty(n * Ls, np.uint8)
    off = np.empty(n + 1, np.uint64)
    abi.check(L.kgx_memcpy_d2h(res.ctypes.data, d_res, res.nbytes), "d2h")
    abi.check(L.kgx_memcpy_d2h(off.ctypes.data, d_off, off.nbytes), "d2h")
    L.kgx_device_free(d_res)
    L.kgx_device_free(d_off)
    params = abi.default_params()
    want = args.want
    t0 = time.time()
    one = ctx0.process_batch(res, off, params, want=want)
    t_one = time.time() - t0
    ctx0.close()
    checks = {}
    with abi.Pool(images, n_ctx=N) as pool:
        got = pool.process_batch(res, off, params, want=want, copy=False)
        checks["hit_offsets"] = bool(np.array_equal(got.hit_offsets, one.hit_offsets))
        checks["hits"] = bool(got.hits.tobytes() == one.hits.tobytes())
        checks["call_offsets"] = bool(np.array_equal(got.call_offsets, one.call_offsets))
        checks["calls"] = bool(got.calls.tobytes() == one.calls.tobytes())
        if one.best is not None:
            checks["best"] = bool(got.best is not None and got.best.tobytes() == one.best.tobytes())
        del got
        ts = []
        r = pool.process_batch_compact(res, off, params, want=want)  # warm
        for _ in range(5):
            t0 = time.perf_counter()
            r = pool.process_batch_compact(res, off, params, want=want)
            ts.append(time.perf_counter() - t0)
        checks["compact_hit_offsets"] = bool(np.array_equal(r.result.hit_offsets, one.hit_offsets))
    t = float(np.median(ts))
    ok = all(checks.values())
    line = {
        "metric": "C5 protein residues/s through kgx_pool, one process over N image replicas",
        "value": n * Ls / t, "unit": "residues/s", "ms_per_batch": t * 1e3, "n_devices": N, "devices": devices,
        "distinct_devices": len(set(devices)), "higher_is_better": True, "dtype": "u64", "data": "synthetic",
        "config": {"workload": f"C5: {n} x {Ls}-aa synthetic proteins, one host batch, vs {n_keys:,}-key image "
                               f"replicated on {N} device slot(s)", "want": want,
                   "outputs": WANT_OUTPUTS.get(want, f"want={want}"), "result": "compact (records + mask)"},
        "match_single_context": ok, "checks": checks, "hits": int(one.hit_offsets[-1]),
        "calls": int(one.call_offsets[-1]), "single_context_s": t_one,
        "image_build_s": t_build, "replicate_s": t_rep,
        "note": "host buffers in and out (PCIe-inclusive); on one GPU the replicas share device 0, so this "
                "exercises the multi-device code path, not N devices' bandwidth",
    }
    print(json.dumps(line), flush=True)
    for im in images:
        im.close()
    if not ok:
        log(f"[pool] MISMATCH against the single-context pass: {checks}")
        return 1
    return 0


def family_kmap(abi, synth, spec, dev, n_fam):
    """The synthetic family DB of tools/bench_server.py --families: family i =
    source protein i of the image (its 292 windows' k-mers), as
    kmer_to_family_id_ (KMAP_SET) on device dev."""
    n_fam = min(n_fam, spec.n_src)
    keys, ids = [], []
    for a in range(0, n_fam, 20000):  # bounded host memory per step
        src = np.arange(a, min(n_fam, a + 20000))
        keys.append(synth.encode_windows(synth.source_residue_codes(src), synth.SRC_WIN).reshape(-1))
        ids.append(np.repeat(src.astype(np.uint32), synth.SRC_WIN))
    fam = abi.Kmap(dev, abi.KMAP_SET)
    fam.add(np.concatenate(keys), np.concatenate(ids))
    return fam, n_fam


def host_path_lookup_leg(abi, synth, img, spec, dev, res_h, off_h, params, n_fam=100000):
    """/lookup in family mode with find_best_match (lookup_request.cc:153-210,
    446-482) from host buffers: kgx_pool_lookup -- residues up, probe + score
    + device find_best_call + on_hit rollups on the device, only the rollup
    rows, offsets and best calls back (nothing per hit crosses PCIe).  Timed
    over pool sizes, pinned and pageable input; a 1,000-sequence slice is
    checked against one context's pass + kgx_kmap_rollup."""
    t0 = time.time()
    fam, n_fam = family_kmap(abi, synth, spec, dev, n_fam)
    t_fam = time.time() - t0
    n = len(off_h) - 1
    n_res = int(off_h[-1] - off_h[0])
    want = abi.WANT_BEST
    pin = abi.pinned_empty(len(res_h))
    pin[:] = res_h
    by, rows_n, ev_n = {}, 0, 0
    best_cfg, best_t = None, None
    for n_ctx in (2, 4, 8):
        with abi.Pool([img], n_ctx) as pool:
            for name, src in (("pinned", pin), ("pageable", res_h)):
                r, roff, rows = pool.lookup([fam], src, off_h, params, want=want, copy=False)  # warm
                ts = []
                for _ in range(7):
                    t1 = time.perf_counter()
                    r, roff, rows = pool.lookup([fam], src, off_h, params, want=want, copy=False)
                    ts.append(time.perf_counter() - t1)
                t = float(np.median(ts))
                by[f"{name}_ctx{n_ctx}"] = t * 1e3
                if name == "pinned" and (best_t is None or t < best_t):
                    best_t, best_cfg = t, n_ctx
            S = min(1000, n)
            sl_off, sl_rows = roff[:S + 1].copy(), rows[:int(roff[S])].copy()
            sl_best = r.best[:S].copy()
            rows_n, ev_n = int(roff[-1]), int(r.hit_offsets[-1])
    with abi.Context(img) as c1:
        one = c1.process_batch(res_h[:int(off_h[S] - off_h[0])], off_h[:S + 1] - off_h[0], params, want=want)
        woff, wrows = fam.rollup(c1, abi.ROLLUP_FAMILY)
    ok = (np.array_equal(sl_off, woff) and sl_rows.tobytes() == wrows.tobytes()
          and sl_best.tobytes() == one.best.tobytes())
    fam.close()
    t_pg = min(v for k, v in by.items() if k.startswith("pageable")) / 1e3
    out = {"value": n_res / best_t, "unit": "residues/s", "ms_per_batch": best_t * 1e3, "pool_contexts": best_cfg,
           "value_pageable_input": n_res / t_pg, "ms_by_config": by,
           "rollup_rows": rows_n, "hits_on_device": ev_n, "families": n_fam, "family_db_build_s": round(t_fam, 2),
           "slice_check": {"sequences": S, "equal_to_one_context_pass_plus_kgx_kmap_rollup": bool(ok)},
           "note": "lookup_request family mode + find_best_match over the C2 batch from host buffers "
                   "(kgx_pool_lookup over one device): H2D residues, probe, score, device find_best_call and the "
                   "on_hit rollups on the device; D2H only rollup rows (16 B each), their offsets and the best "
                   "calls.  value: residues in pinned memory (kgx_host_alloc, read by DMA, no staging); "
                   "value_pageable_input: the same from pageable memory (staged).  Parity of the rows against "
                   "on_hit over the oracle's hits: tests/test_gpu_lookup_pool.py"}
    log(f"[bench] host_path_lookup {out['value']:.3e} residues/s ({best_t * 1e3:.2f} ms, {best_cfg} contexts), "
        f"pageable {out['value_pageable_input']:.3e}; slice check {'ok' if ok else 'MISMATCH'}; {by}")
    return out


def pool_devices(dev: int, n_dev: int, world: int) -> list:
    """The pool_e2e leg's devices: this rank's first, then as many of the
    other visible devices as the job has ranks (an N-GPU run measures C5 over
    N devices; the one-GPU run over one)."""
    return [dev] + [i for i in range(n_dev) if i != dev][:max(0, world - 1)]


GB = 1e9
RANK_HBM = 8e9   # a rank's batches and worker contexts (C2), with room to spare
POOL_HBM = 24e9  # the C5 legs per device: pool contexts (1M x 300 aa), family map, one-pass reference


def image_bytes(n_keys: int, num_sigs: int, line_load: int) -> dict:
    """HBM an image of the bench takes: the file's 24-B buckets while it is
    built, its PACKED16 records, and the line index (stored keys x 64 / load
    lines of 64 B)."""
    lines = (n_keys * 64 + line_load - 1) // line_load if line_load else 0
    return {"aos24": num_sigs * 24, "packed16": num_sigs * 16, "line_index": lines * 64}


def hbm_check(abi, devices, need: float, what: str) -> None:
    """Fail with a clear message when a device has less free HBM than need."""
    for dv in devices:
        free, total = abi.device_memory(dv)
        if free < need:
            raise SystemExit(f"device {dv}: {free / GB:.1f} GB of {total / GB:.1f} GB HBM free, but {what} needs "
                             f"{need / GB:.1f} GB")


def c5_batch(abi, L, img0, spec, n, Ls, x_permille):
    """BASELINE.json configs[4]'s batch (C5: n x Ls aa), generated on img0's
    device and copied into pinned host memory: (residues, offsets)."""
    c0 = abi.Context(img0)
    dev = img0.device
    d_res, d_off = ctypes.c_void_p(), ctypes.c_void_p()
    abi.check(L.kgx_device_alloc(dev, n * Ls, ctypes.byref(d_res)), "alloc")
    abi.check(L.kgx_device_alloc(dev, (n + 1) * 8, ctypes.byref(d_off)), "alloc")
    abi.check(L.kgx_synth_queries(c0.handle, spec.n_keys, n, Ls, x_permille, 1 << 40, d_res, d_off), "queries")
    c0.synchronize()
    pin = abi.pinned_empty(n * Ls)
    off = np.empty(n + 1, np.uint64)
    abi.check(L.kgx_memcpy_d2h(pin.ctypes.data, d_res, pin.nbytes), "d2h")
    abi.check(L.kgx_memcpy_d2h(off.ctypes.data, d_off, off.nbytes), "d2h")
    L.kgx_device_free(d_res)
    L.kgx_device_free(d_off)
    c0.close()
    return pin, off


def pool_e2e_leg(abi, images, pin, off, params, want):
    """C5 (BASELINE.json configs[4]) as the reference would run it: one host
    batch through kgx_pool over one image replica per device (images: rank
    0's image, then device-to-device copies of it), residue-balanced shards,
    compact results concatenated in input order (threadpool.cc:18-44,
    lookup_request.cc:153).  Timed over contexts per device, pinned and
    pageable input; checked against one context's pass over the batch."""
    devices = [im.device for im in images]
    n = len(off) - 1
    n_res = int(off[-1] - off[0])
    pageable = np.array(pin)
    c0 = abi.Context(images[0])
    one = c0.process_batch_compact(pageable, off, params, want=want)
    one_off = (one.result.hit_offsets.copy(), one.result.call_offsets.copy(), one.result.calls.copy(),
               one.result.best.copy() if one.result.best is not None else None)
    rng = np.random.default_rng(5)
    starts = sorted(set([0, n - 500] + rng.integers(0, n - 500, 12).tolist()))
    one_hits = {a: one.expand(a, a + 500).tobytes() for a in starts}
    c0.close()
    by, checks, numa = {}, {}, None
    best_t, best_k = None, None
    for per_dev in (1, 2, 4, 8):
        n_ctx = per_dev * len(devices)
        with abi.Pool(images, n_ctx) as pool:
            if numa is None:
                numa = pool.numa_nodes()[:len(devices)]
            for name, src in (("pinned", pin), ("pageable", pageable)):
                r = pool.process_batch_compact(src, off, params, want=want)  # warm
                ts = []
                for _ in range(5):
                    t1 = time.perf_counter()
                    r = pool.process_batch_compact(src, off, params, want=want)
                    ts.append(time.perf_counter() - t1)
                t = float(np.median(ts))
                by[f"{name}_ctx{n_ctx}"] = t * 1e3
                if name == "pinned" and (best_t is None or t < best_t):
                    best_t, best_k = t, n_ctx
                rr = r.result
                ok = (np.array_equal(rr.hit_offsets, one_off[0]) and np.array_equal(rr.call_offsets, one_off[1])
                      and rr.calls.tobytes() == one_off[2].tobytes()
                      and (one_off[3] is None or rr.best.tobytes() == one_off[3].tobytes())
                      and all(r.expand(a, a + 500).tobytes() == one_hits[a] for a in starts))
                checks[f"{name}_ctx{n_ctx}"] = bool(ok)
    t_pg = min(v for k, v in by.items() if k.startswith("pageable")) / 1e3
    out = {"value": n_res / best_t, "unit": "residues/s", "ms_per_batch": best_t * 1e3, "contexts": best_k,
           "devices": devices, "numa_nodes": numa, "value_pageable_input": n_res / t_pg, "ms_by_config": by,
           "match_single_context": all(checks.values()), "checks": checks,
           "hits": int(one_off[0][-1]),
           "note": "C5: one host batch through kgx_pool_process_batch_compact over one image replica per device "
                   "(hits as compact records + mask, calls, device best calls back over PCIe), contexts per device "
                   "swept; value: residues in pinned memory (read by DMA, no staging copy); checked against one "
                   "context's pass (offsets, calls, best calls, and the expanded hits of 14 slices of 500 "
                   "sequences, shard cuts included); numa_nodes: the node each device's first pool thread is "
                   "bound to (-1 unbound)"}
    log(f"[bench] pool_e2e {out['value']:.3e} residues/s over {len(devices)} device(s) ({best_k} contexts, "
        f"{best_t * 1e3:.1f} ms), pageable {out['value_pageable_input']:.3e}; checks "
        f"{'ok' if out['match_single_context'] else checks}; numa {numa}; {by}")
    return out


def pool_lookup_leg(abi, synth, images, spec, pin, off, params, n_fam=100000):
    """/lookup in family mode with find_best_match (lookup_request.cc:153-210,
    446-482, the north_star handler) over C5's batch and every device of the
    pool: kgx_pool_lookup with one family map per device (kgx_kmap on each
    replica's device), rows + offsets + best calls back.  Timed at 4 and 8
    contexts per device, pinned and pageable input; the whole batch's rows,
    offsets and best calls are checked byte for byte against one context's
    one-pass run + kgx_kmap_rollup."""
    devices = [im.device for im in images]
    n = len(off) - 1
    n_res = int(off[-1] - off[0])
    want = abi.WANT_BEST
    t0 = time.time()
    fams = [family_kmap(abi, synth, spec, dv, n_fam)[0] for dv in devices]
    t_fam = time.time() - t0
    pageable = np.array(pin)
    with abi.Context(images[0]) as c1:
        c1.set_option("host_chunks", 1)  # the rollup reads the pass's hits on the device
        one = c1.process_batch(pageable, off, params, want=want)
        woff, wrows = fams[0].rollup(c1, abi.ROLLUP_FAMILY)
        wbest = one.best.copy()
        del one
    by, checks = {}, {}
    best_t, best_k = None, None
    for per_dev in (4, 8):
        n_ctx = per_dev * len(devices)
        with abi.Pool(images, n_ctx) as pool:
            for name, src in (("pinned", pin), ("pageable", pageable)):
                r, roff, rows = pool.lookup(fams, src, off, params, want=want, copy=False)  # warm
                ts = []
                for _ in range(5):
                    t1 = time.perf_counter()
                    r, roff, rows = pool.lookup(fams, src, off, params, want=want, copy=False)
                    ts.append(time.perf_counter() - t1)
                t = float(np.median(ts))
                by[f"{name}_ctx{n_ctx}"] = t * 1e3
                if name == "pinned" and (best_t is None or t < best_t):
                    best_t, best_k = t, n_ctx
                checks[f"{name}_ctx{n_ctx}"] = bool(np.array_equal(roff, woff) and rows.tobytes() == wrows.tobytes()
                                                    and r.best.tobytes() == wbest.tobytes())
    for f in fams:
        f.close()
    t_pg = min(v for k, v in by.items() if k.startswith("pageable")) / 1e3
    out = {"value": n_res / best_t, "unit": "residues/s", "ms_per_batch": best_t * 1e3, "contexts": best_k,
           "devices": devices, "value_pageable_input": n_res / t_pg, "ms_by_config": by,
           "rollup_rows": int(woff[-1]), "families": n_fam, "family_db_build_s": round(t_fam, 2),
           "match_single_context": all(checks.values()), "checks": checks,
           "check": f"all {n} sequences' rollup offsets, rows and best calls == one context's one-pass run + "
                    "kgx_kmap_rollup",
           "note": "C5 /lookup (family mode + find_best_match, the north_star handler) through kgx_pool_lookup "
                   "over one image replica and one family map per device: residues up, probe, score, device "
                   "find_best_call and on_hit rollups on each device, only rows, offsets and best calls back"}
    log(f"[bench] pool_lookup {out['value']:.3e} residues/s over {len(devices)} device(s) ({best_k} contexts, "
        f"{best_t * 1e3:.2f} ms), pageable {out['value_pageable_input']:.3e}; checks "
        f"{'ok' if out['match_single_context'] else checks}; {by}")
    return out


DUMP_SEQS = 4096        # sequences of the seeded sample whose rows are written
DUMP_SEED = 0x6b6778    # fixed: the same sequences in every run of the same arguments
DUMP_CAP = 64 << 20     # bytes, all files together


def _as_float(a: np.ndarray) -> np.ndarray:
    """a as float32 where that is exact for its type (float32, <= 16-bit
    integers), else float64 (32-bit integers; the k-mer keys are < 20^8)."""
    exact32 = (a.dtype.kind == "f" and a.dtype.itemsize <= 4) or (a.dtype.kind in "iu" and a.dtype.itemsize <= 2)
    return np.ascontiguousarray(a, dtype=np.float32 if exact32 else np.float64)


def dump_arrays(got, n_sample: int = DUMP_SEQS, cap: int = DUMP_CAP) -> dict:
    """The arrays --dump-outputs writes, from the host CSR results of one step
    (got: hit_offsets / hits, call_offsets / calls, best): every sequence's
    hit and call count, and for a seeded sample of sequences (sample_seq,
    ascending) their hits, calls and best calls, one array per record field,
    rows in sequence order.  The sample is halved until all fit in cap."""
    n = len(got.hit_offsets) - 1
    ho = np.asarray(got.hit_offsets, np.int64)
    co = np.asarray(got.call_offsets, np.int64)
    out = {"hit_counts": np.diff(ho).astype(np.float32), "call_counts": np.diff(co).astype(np.float32)}
    fixed = sum(a.nbytes for a in out.values())
    k = min(n, n_sample)
    while True:
        sample = np.zeros(0, np.int64)
        if k:
            sample = np.sort(np.random.default_rng(DUMP_SEED).choice(n, k, replace=False))
        part = {"sample_seq": sample.astype(np.float64)}
        for name, off, rows in (("hits", ho, got.hits), ("calls", co, got.calls)):
            idx = np.concatenate([np.arange(off[s], off[s + 1]) for s in sample] + [np.zeros(0, np.int64)])
            # the sample's own CSR: sequence sample_seq[i] owns rows [offsets[i], offsets[i + 1])
            part[f"{name}_offsets"] = np.concatenate([[0], np.cumsum(off[sample + 1] - off[sample])]).astype(np.float64)
            for f in rows.dtype.names:
                part[f"{name}_{f}"] = _as_float(rows[f][idx])
        if got.best is not None:
            for f in got.best.dtype.names:
                part[f"best_{f}"] = _as_float(got.best[f][sample])
        if fixed + sum(a.nbytes for a in part.values()) <= cap or k == 0:
            break
        k //= 2
    out.update(part)
    return out


def dump_outputs(path: str, got, rank: int = 0, world: int = 1) -> int:
    """Write dump_arrays(got) as path/<name>.npy (rank r of a multi-rank job:
    path/rank<r>_<name>.npy, its own shard); returns the bytes written."""
    os.makedirs(path, exist_ok=True)
    arrays = dump_arrays(got)
    for name, a in arrays.items():
        np.save(os.path.join(path, (f"rank{rank}_" if world > 1 else "") + name + ".npy"), a)
    return sum(a.nbytes for a in arrays.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n-keys", type=float, default=1e9, help="distinct keys stored in the image")
    ap.add_argument("--num-sigs", type=int, default=0, help="0 = builder sizing rule")
    ap.add_argument("--n-seq", type=int, default=100000, help="sequences per GPU (C2) / per batch (--strong)")
    ap.add_argument("--strong", action="store_true",
                    help="C5: one batch of --strong-seq proteins split across the ranks (strong scaling)")
    ap.add_argument("--strong-seq", type=int, default=1000000)
    ap.add_argument("--batches", type=int, default=8, help="distinct resident batches the steps rotate over")
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--x-permille", type=int, default=0)
    ap.add_argument("--cpu-sample", type=int, default=100000)
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="0 = the CPUs this process may use (affinity mask, capped by a cgroup quota)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-microbench", action="store_true")
    ap.add_argument("--no-host-path", action="store_true")
    ap.add_argument("--no-lookup", action="store_true", help="skip the host_path_lookup leg")
    ap.add_argument("--no-pool", action="store_true", help="skip the pool_e2e leg (C5 through kgx_pool)")
    ap.add_argument("--no-pool-lookup", action="store_true",
                    help="skip the pool_lookup leg (C5 /lookup through kgx_pool_lookup over the devices)")
    ap.add_argument("--families", type=int, default=100000, help="family DB size of the host_path_lookup leg")
    ap.add_argument("--ab", default="", help='interleaved A/B of a ctx option, e.g. "probe_j=4,5,8"')
    ap.add_argument("--ab-rounds", type=int, default=10)
    ap.add_argument("--pipeline", type=int, default=2, help="worker contexts (streams) in flight")
    ap.add_argument("--ctx-option", action="append", default=[],
                    help="name=value context option for every worker context (repeatable; tuning A/Bs)")
    ap.add_argument("--filter-log2", type=int, default=0,
                    help="presence filter of 2^N bits (0 = none), kgx_image_set_filter")
    ap.add_argument("--image-layout", choices=["packed", "aos"], default="packed",
                    help="HBM-resident bucket layout (packed when the payloads fit)")
    ap.add_argument("--line-index", type=int, default=36,
                    help="kgx_image_set_line_index load, keys per 64 lines (default 36: 9/16 of a key per "
                         "64-B line, 114 GB beside the 57-GB packed table at C2; 0 = probe the reference slots)")
    ap.add_argument("--want", type=int, default=11,
                    help="KGX_WANT_* mask (11 = hits + calls + device best call, lookup_request find_best_match)")
    ap.add_argument("--no-canary", action="store_true", help="skip the per-device canary self-check")
    ap.add_argument("--no-parity", action="store_true",
                    help="skip the full-batch check of the timed configuration against the oracle")
    ap.add_argument("--line-index-ab", type=int, default=10,
                    help="rounds of the in-process line-index A/B (option line_index 0 / 1 over the same "
                         "batches, interleaved; 0 = skip)")
    ap.add_argument("--ab-steps", type=int, default=40, help="steps per A/B sample")
    ap.add_argument("--pipe-ab", default="",
                    help='interleaved A/B of a context option over pipelined steps, e.g. "probe_nt=0,1" '
                         '(the first value stays set afterwards)')
    ap.add_argument("--pool-devices", type=int, default=0,
                    help="N > 0: one process, the C5 batch through kgx_pool over N image replicas (devices "
                         "i %% visible), checked byte for byte against one context; prints its own line")
    ap.add_argument("--probe-lds-kb", type=int, default=-1, help="LDS KB reserved per probe workgroup (-1 = default)")
    ap.add_argument("--probe-stream", type=int, default=-1,
                    help="1 = the contexts' chained probes on one image stream (-1 = default)")
    ap.add_argument("--probe-persist", type=int, default=-1,
                    help="line-probe grid cap in workgroups per CU, waves striding over tiles (-1 = default)")
    ap.add_argument("--score-variant", type=int, default=0, help="0 = hybrid (default: lanes, long sequences on the wave scorer), 1 = wave-parallel, 2 = lanes only")
    ap.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "probe_traffic.json"))
    ap.add_argument("--full", action="store_true",
                    help="beside the timed steps: the canary self-check, the probe / score kernel times and the "
                         "roofline, the parity check against the oracle, the host-path, lookup and pool legs, the "
                         "random-read microbenchmark and the CPU baseline (each with its --no-* switch); without "
                         "it a run builds the image, settles the line index, warms up, times --steps steps and "
                         "prints the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="write what the last timed step computed (the host CSR results a caller collects: "
                         "per-sequence counts, and the hits, calls and best calls of a fixed seeded sample of "
                         "sequences) as DIR/<name>.npy, float32 / float64, at most 64 MB")
    args = ap.parse_args()

    from close_kmers_amd import shard

    if args.pool_devices:
        sys.exit(pool_main(args))
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ:
        if args.gpus > 1:
            # --gpus N without torchrun: start the N ranks here, one process
            # per GPU, before anything in this process touches the GPU; rank
            # 0's JSON line is relayed, a failing rank fails the job
            cmd = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]
            sys.exit(shard.launch_ranks(cmd, args.gpus))
    elif int(os.environ["WORLD_SIZE"]) != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but the launcher started {os.environ['WORLD_SIZE']} ranks")

    # one GPU per rank; KGX_BENCH_DEVICE pins every rank to one device (a
    # rehearsal of the multi-rank control flow on a 1-GPU box, small images)
    dev = int(os.environ.get("KGX_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))
    from close_kmers_amd import abi, synth
    L = abi.lib()
    n_dev = abi.device_count()
    if n_dev <= dev:
        raise SystemExit(f"rank {os.environ.get('RANK', '0')}: no device {dev} "
                         f"({n_dev} gfx950 device(s) visible)")

    d = shard.Dist()
    canary_recs = None
    if args.full and not args.no_canary:
        canary_recs, canary_ok = canary_check(abi, synth, d, dev,
                                              args.line_index if args.image_layout == "packed" else 0)
        if not canary_ok:
            d.close()
            raise SystemExit(f"rank {d.rank}: canary check failed (a device's results differ from the oracle's)")
    n_keys = int(args.n_keys)
    spec = synth.ImageSpec(n_keys, args.num_sigs or None)

    # HBM budget of this rank's image before building it: the 24-B build, then
    # PACKED16 and the line index beside it, plus the batches and contexts
    img_bytes = image_bytes(n_keys, spec.num_sigs, args.line_index if args.image_layout == "packed" else 0)
    peak = max(img_bytes["aos24"] + (img_bytes["packed16"] if args.image_layout == "packed" else 0),
               img_bytes["packed16"] + img_bytes["line_index"]) + RANK_HBM
    hbm_check(abi, [dev], peak, f"rank {d.rank}'s image (built as {img_bytes['aos24'] / GB:.1f} GB of 24-B "
                                f"buckets, kept as {img_bytes['packed16'] / GB:.1f} GB PACKED16 + "
                                f"{img_bytes['line_index'] / GB:.1f} GB line index) and its batches")
    t0 = time.time()
    # n_keys distinct keys stored (the generator's stream
    # runs past n_keys entries until that many distinct keys are in)
    img, n_entries = abi.Image.synthetic_distinct(spec.n_keys, n_keys, spec.num_sigs, device=dev)
    stored = n_keys
    log(f"[bench] rank {d.rank}: built {stored} distinct keys ({n_entries} entries of the stream) in "
        f"{spec.num_sigs} buckets ({spec.num_sigs * 24 / 1e9:.1f} GB) on device {dev} in {time.time() - t0:.1f}s")
    if args.image_layout == "aos":
        img.set_layout(abi.Image.AOS24)
    line_lines = 0
    if args.line_index and img.layout == abi.Image.PACKED16:
        t0 = time.time()
        img.set_line_index(args.line_index)
        line_lines = img.line_count
        log(f"[bench] line index: {line_lines:,} lines ({line_lines * 64 / 1e9:.1f} GB) "
            f"in {time.time() - t0:.1f}s")
    if args.filter_log2:
        t0 = time.time()
        img.set_filter(args.filter_log2)
        log(f"[bench] presence filter 2^{args.filter_log2} bits built in {time.time() - t0:.2f}s")
    layout = ["AOS24", "PACKED16"][img.layout]
    # the default probe (probe_variant -1): cooperative lines for PACKED16 without a filter
    probe_kernel = "probe_line_kernel" if layout == "PACKED16" and not args.filter_log2 else "probe_kernel"
    log(f"[bench] resident layout {layout}")
    ctx = abi.Context(img)
    Ls = args.length

    # this rank's queries: weak (C2) = its own n_seq per batch; strong (C5) =
    # its residue-balanced shard of each global batch (all lengths equal, so
    # balanced_shards cuts equal counts)
    if args.strong:
        n_global = args.strong_seq
        glob_off = np.arange(n_global + 1, dtype=np.uint64) * np.uint64(Ls)
        s0, s1 = shard.balanced_shards(glob_off, d.world)[d.rank]
        n = s1 - s0
        q0s = [b * n_global + s0 for b in range(args.batches)]
    else:
        n_global = args.n_seq * d.world
        n = args.n_seq
        q0s = [(b * d.world + d.rank) * n for b in range(args.batches)]
    if n < 1:
        raise SystemExit(f"rank {d.rank}: empty shard")
    n_res = n * Ls
    batches = []
    for q0 in q0s:
        d_res, d_off = ctypes.c_void_p(), ctypes.c_void_p()
        abi.check(L.kgx_device_alloc(dev, n_res, ctypes.byref(d_res)), "alloc residues")
        abi.check(L.kgx_device_alloc(dev, (n + 1) * 8, ctypes.byref(d_off)), "alloc offsets")
        abi.check(L.kgx_synth_queries(ctx.handle, spec.n_keys, n, Ls, args.x_permille, q0, d_res, d_off),
                  "synth queries")
        batches.append((d_res, d_off))
    ctx.synchronize()

    params = abi.default_params()
    # lookup_request.cc:166-172 (find_best_match in family mode): hits through
    # on_hit + the calls vector, no OTU stats; --want 7 adds OTU (/add)
    want = args.want
    ev = [ctypes.c_void_p() for _ in range(4)]
    for e in ev:
        abi.check(L.kgx_event_create(ctypes.byref(e)), "event")

    # worker contexts: like the reference's thread pool (one KmerGuts per
    # worker over one shared image, threadpool.cc:18-44), each has its own
    # stream and buffers, so one worker's scoring overlaps the next worker's
    # probe.  Every step is still a full pass over a whole batch.
    ctxs = [ctx] + [abi.Context(img) for _ in range(args.pipeline - 1)]
    for c in ctxs:
        c.set_option("score_variant", args.score_variant)
        if args.probe_lds_kb >= 0:
            c.set_option("probe_lds_kb", args.probe_lds_kb)
        if args.probe_persist >= 0:
            c.set_option("probe_persist", args.probe_persist)
        if args.probe_stream >= 0:
            c.set_option("probe_stream", args.probe_stream)
        for o in args.ctx_option:
            name, value = o.split("=")
            c.set_option(name, int(value))
    score_ms: list = []  # score stage (+ best/OTU kernels with --want), same untimed pass as probe_ms

    def step(timed_probe: list | None, c=ctx, b=0):
        d_res, d_off = batches[b % len(batches)]
        abi.check(L.kgx_stage_plan(c.handle, d_off, n, n_res), "plan")
        if timed_probe is not None:
            abi.check(L.kgx_event_record(ev[0], c.handle), "event")
        abi.check(L.kgx_stage_probe(c.handle, d_res, d_off), "probe")
        if timed_probe is not None:
            abi.check(L.kgx_event_record(ev[1], c.handle), "event")
        abi.check(L.kgx_stage_score(c.handle, ctypes.byref(params), want), "score")
        if timed_probe is not None:
            abi.check(L.kgx_event_record(ev[2], c.handle), "event")
            ms, ms2 = ctypes.c_float(), ctypes.c_float()
            abi.check(L.kgx_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
            abi.check(L.kgx_event_elapsed_ms(ev[1], ev[2], ctypes.byref(ms2)), "elapsed")
            timed_probe.append(ms.value)
            score_ms.append(ms2.value)

    for i in range(args.warmup * len(ctxs)):
        step(None, ctxs[i % len(ctxs)], i)
    for c in ctxs:
        c.synchronize()

    # probe-kernel duration (HIP events on the context's stream), untimed
    # pass, rotating over the batches like the timed steps (--full: the
    # roofline's kernel time)
    probe_ms: list = []
    if args.full:
        for i in range(max(3, min(args.steps, 10))):
            step(probe_ms, ctx, i)
        ctx.synchronize()

    probe_ab = None
    if args.ab:
        # interleaved A/B of one tuning option in this process (one process,
        # alternating rounds, report the distribution); "name=v1,v2,..."
        # several options at once: "probe_variant,probe_j=-1:4,2:4,3:2"
        name, vals = args.ab.split("=")
        names = name.split(",")
        vals = vals.split(",")
        times = {v: [] for v in vals}
        stimes = {v: [] for v in vals}
        k = 0
        for _ in range(args.ab_rounds):
            for v in vals:
                for nm, x in zip(names, v.split(":")):
                    ctx.set_option(nm, int(x))
                step(times[v], ctx, k)
                stimes[v].append(score_ms.pop())
                k += 1
        ctx.set_option("probe_variant", -1)
        ctx.set_option("probe_j", 2)
        ctx.set_option("probe_filter", 1)
        probe_ab = {"option": name,
                    **{str(v): {"median_ms": float(np.median(t)), "min_ms": float(np.min(t)),
                                "score_median_ms": float(np.median(stimes[v]))}
                       for v, t in times.items()}}
        log(f"[bench] probe A/B: {probe_ab}")

    def pipelined_ab(name, values, rounds, restore):
        """Interleaved A/B of a context option over the timed loop's shape:
        the same batches and worker contexts, each sample a run of
        --ab-steps pipelined steps (wall clock) plus one event-timed probe,
        the values' order alternating by round so drift hits all alike."""
        samples = {v: {"step": [], "probe": []} for v in values}
        k = 0
        for r in range(rounds):
            for v in (values if r % 2 == 0 else values[::-1]):
                for c in ctxs:
                    c.set_option(name, v)
                for i in range(len(ctxs)):  # settle the rotation
                    step(None, ctxs[i % len(ctxs)], k)
                    k += 1
                for c in ctxs:
                    c.synchronize()
                t1 = time.perf_counter()
                for i in range(args.ab_steps):
                    step(None, ctxs[i % len(ctxs)], k)
                    k += 1
                for c in ctxs:
                    c.synchronize()
                samples[v]["step"].append((time.perf_counter() - t1) * 1e3 / args.ab_steps)
                pm: list = []
                step(pm, ctx, k)
                k += 1
                ctx.synchronize()
                score_ms.pop()
                samples[v]["probe"].append(pm[0])
        for c in ctxs:
            c.set_option(name, restore)
        return {str(v): {"median_step_ms": float(np.median(samples[v]["step"])),
                         "median_probe_ms": float(np.median(samples[v]["probe"])),
                         "step_ms": [round(x, 4) for x in samples[v]["step"]],
                         "probe_ms": [round(x, 4) for x in samples[v]["probe"]]} for v in values}

    # the line index, settled in this process before the timed steps: option
    # line_index 0 (probes over the reference slots) and 1 (the index) on the
    # same batches; the timed steps then run the faster of the two on this
    # box (round 6 measured +11.6% .. -0.3% across seven boxes)
    line_ab = None
    use_index = 1 if line_lines else 0
    if line_lines and args.line_index_ab > 0:
        med = pipelined_ab("line_index", [0, 1], args.line_index_ab, 1)
        gain = med["0"]["median_step_ms"] / med["1"]["median_step_ms"] - 1.0
        use_index = 1 if gain >= 0 else 0
        for c in ctxs:
            c.set_option("line_index", use_index)
        line_ab = {"rounds": args.line_index_ab, "steps_per_sample": args.ab_steps, "load": args.line_index,
                   "without_index": med["0"], "with_index": med["1"],
                   "step_gain": gain, "timed_with_index": bool(use_index),
                   "note": "one process, same batches and worker contexts, before the timed steps; context option "
                           "line_index 0 = probes over the reference slots, 1 = over the line index; step_gain = "
                           "without / with - 1; the timed steps, the probe time and the parity check use the faster"}
        log(f"[bench] line index A/B ({args.line_index_ab} rounds): step {med['0']['median_step_ms']:.4f} ms "
            f"without, {med['1']['median_step_ms']:.4f} with ({gain * 100:+.1f}%); probe "
            f"{med['0']['median_probe_ms']:.4f} / {med['1']['median_probe_ms']:.4f} ms; timed "
            f"{'with' if use_index else 'without'} the index")
        if args.full and not use_index:  # the probe time under the timed configuration
            probe_ms.clear()
            for i in range(max(3, min(args.steps, 10))):
                step(probe_ms, ctx, i)
            ctx.synchronize()
    timed_load = args.line_index if (line_lines and use_index) else 0
    pipe_ab = None
    if args.pipe_ab:
        name, vals = args.pipe_ab.split("=")
        values = [int(x) for x in vals.split(",")]
        pipe_ab = {"option": name, **pipelined_ab(name, values, args.ab_rounds, values[0])}
        log(f"[bench] pipelined A/B of {name}: " + ", ".join(
            f"{v}: step {pipe_ab[str(v)]['median_step_ms']:.4f} probe {pipe_ab[str(v)]['median_probe_ms']:.4f} ms"
            for v in values))

    d.barrier()
    for c in ctxs:
        c.synchronize()
    t_start = time.perf_counter()
    for i in range(args.steps):
        step(None, ctxs[i % len(ctxs)], i)
    for c in ctxs:
        c.synchronize()
    d.barrier()
    t_wall = time.perf_counter() - t_start
    t_max = d.max(t_wall)
    last = ctxs[(args.steps - 1) % len(ctxs)]

    # sanity: counts of the last step
    out = abi.DeviceResult()
    abi.check(L.kgx_device_result_get(last.handle, ctypes.byref(out)), "result")
    last.check_plan()
    hc = np.empty(n, np.uint32)
    cc = np.empty(n, np.uint32)
    abi.check(L.kgx_memcpy_d2h(hc.ctypes.data, out.hit_count, hc.nbytes), "d2h")
    abi.check(L.kgx_memcpy_d2h(cc.ctypes.data, out.call_count, cc.nbytes), "d2h")
    total_hits = int(d.sum(float(hc.sum())))
    probe_mean = float(np.mean(probe_ms)) if probe_ms else None  # None without --full
    mine = {"rank": d.rank, "device": dev, "ms_per_step": t_wall * 1e3 / args.steps,
            "probe_ms": probe_mean, "n_seq": n, "hits": int(hc.sum())}
    if canary_recs:
        c = canary_recs[d.rank]
        mine["canary"] = {"ok": c["ok"], "digest": c["digest"][:16], "hits": c["hits"], "calls": c["calls"]}
    per_rank = d.gather_objects(mine)
    log(f"[bench] rank {d.rank}: hits {int(hc.sum())} calls {int(cc.sum())} "
        f"(even-q mean {hc[::2].mean():.1f}, odd-q mean {hc[1::2].mean():.2f}); "
        f"wall {t_wall * 1e3 / args.steps:.3f} ms/step ({len(ctxs)} worker contexts, {len(batches)} batches)"
        + (f", probe {probe_mean:.3f} ms" if probe_ms else ""))

    # --dump-outputs: the last timed step's results, collected from the
    # context that ran it before any later pass reuses its buffers
    if args.dump_outputs:
        t0 = time.time()
        r = abi.Result()
        abi.check(L.kgx_device_batch_collect(last.handle, want, ctypes.byref(r)), "collect")
        nb = dump_outputs(args.dump_outputs, abi.BatchResult(r, want, copy=False), d.rank, d.world)
        log(f"[bench] rank {d.rank}: outputs of timed step {args.steps - 1} (batch "
            f"{(args.steps - 1) % len(batches)}) written, {nb / 1e6:.1f} MB in {time.time() - t0:.1f}s")

    # the timed configuration's results of batch 0, for the full-batch check
    # against the oracle below (rank 0)
    got0 = res0 = off0 = None
    if d.rank == 0 and args.full and not args.no_parity:
        step(None, ctx, 0)
        r = abi.Result()
        abi.check(L.kgx_device_batch_collect(ctx.handle, want, ctypes.byref(r)), "collect")
        got0 = abi.BatchResult(r, want)
        d_res, d_off = batches[0]
        res0 = np.empty(n_res, np.uint8)
        off0 = np.empty(n + 1, np.uint64)
        abi.check(L.kgx_memcpy_d2h(res0.ctypes.data, d_res, res0.nbytes), "d2h")
        abi.check(L.kgx_memcpy_d2h(off0.ctypes.data, d_off, off0.nbytes), "d2h")

    released = []

    def release():
        """This rank's HBM back: events, batches, worker contexts, image."""
        if released:
            return
        released.append(True)
        for e in ev:
            L.kgx_event_destroy(e)
        for d_res, d_off in batches:
            L.kgx_device_free(d_res)
            L.kgx_device_free(d_off)
        for c in ctxs:
            c.close()
        img.close()

    # the other ranks are done with the GPU: they free their HBM before rank
    # 0's C5 legs put image replicas on their devices
    if d.world > 1:
        if d.rank != 0:
            release()
        d.barrier()

    # PCIe-inclusive rate of the host-buffer boundary (kgx_process_batch:
    # H2D residues, plan/probe/score, gather, D2H hits + calls) -- reported
    # beside `value`, never as it
    host_path = None
    if d.rank == 0 and args.full and not args.no_host_path:
        d_res, d_off = batches[0]
        res_h = np.empty(n_res, np.uint8)
        off_h = np.empty(n + 1, np.uint64)
        abi.check(L.kgx_memcpy_d2h(res_h.ctypes.data, d_res, res_h.nbytes), "d2h")
        abi.check(L.kgx_memcpy_d2h(off_h.ctypes.data, d_off, off_h.nbytes), "d2h")
        by_cfg, profiles = {}, {}
        # option tuples (host_chunks, host_hits16, host_stream, compact): the
        # round-1 schedule (3 chunks, 32-B records, host round trip per chunk),
        # the streamed schedule with kgx_hit expanded on host threads, and the
        # compact result (kgx_process_batch_compact: the records + mask the
        # facade replays hit_cb from, no kgx_hit array) -- reported as value
        cfgs = {"one_pass": (1, 1, 1, 0), "r1_exact_32B": (3, 0, 0, 0), "exact_16B": (6, 1, 0, 0),
                "expanded": (6, 1, 1, 0), "compact": (6, 1, 1, 1)}
        for name, (k, h16, hs, cp) in cfgs.items():
            ctx.set_option("host_chunks", k)
            ctx.set_option("host_hits16", h16)
            ctx.set_option("host_stream", hs)
            run = ((lambda: ctx.process_batch_compact(res_h, off_h, params, want=want)) if cp else
                   (lambda: ctx.process_batch(res_h, off_h, params, want=want, copy=False)))
            r = run()  # warm (buffer growth)
            th, pr = [], []
            for _ in range(9):  # timed without the per-chunk timing events
                t0 = time.perf_counter()
                r = run()
                th.append(time.perf_counter() - t0)
            by_cfg[name] = float(np.median(th))
            ctx.set_option("host_profile", 1)  # then the stage profile, in runs of their own
            for _ in range(3):
                r = run()
                pr.append(ctx.host_profile())
            ctx.set_option("host_profile", 0)
            if pr[0]["streamed"]:
                profiles[name] = {k2: float(np.median([q[k2] for q in pr])) for k2 in pr[0]}
        t_h = by_cfg["compact"]
        t_x = by_cfg["expanded"]
        rr = r.result
        n_hits, n_calls = int(rr.hit_offsets[-1]), int(rr.call_offsets[-1])
        mask_bytes = n_res // 8  # the hit mask: one bit per window
        host_path = {"value": n_res / t_h, "unit": "residues/s", "ms_per_batch": t_h * 1e3,
                     "value_kgx_hit": n_res / t_x, "ms_per_batch_kgx_hit": t_x * 1e3,
                     "ms_per_batch_by_schedule": {k: v * 1e3 for k, v in by_cfg.items()},
                     "schedules": {k: dict(zip(("host_chunks", "host_hits16", "host_stream", "compact"), v))
                                   for k, v in cfgs.items()},
                     "stage_profile_ms": profiles,
                     "d2h_bytes": int(n_hits * 12 + mask_bytes + n_calls * 20),
                     "d2h_bytes_32B_records": int(n_hits * 32 + n_calls * 20),
                     "note": "host buffers in, host results out (PCIe-inclusive): H2D residues + kernels + D2H "
                             "into pinned host memory.  6 chunks over two contexts, device CSR offsets, bulk "
                             "copies on a copy stream sized on the device, 12-B records (no key) + the hit mask "
                             "over PCIe.  value: kgx_process_batch_compact (records + mask, what the facade "
                             "replays hit_cb from); value_kgx_hit: kgx_process_batch, 32-B kgx_hit records built "
                             "by host threads while later chunks stream.  stage_profile_ms: HIP-event sums per "
                             "stage over the chunks (they overlap) and host wall times, from separate runs with host_profile 1 "
                             "(the timed runs record no per-chunk events)"}
        log(f"[bench] host-buffer path {n_res / t_h:.3e} residues/s compact ({t_h * 1e3:.2f} ms/batch), "
            f"{n_res / t_x:.3e} with kgx_hit ({t_x * 1e3:.2f} ms); profiles {profiles}")

    host_path_lookup = None
    if d.rank == 0 and args.full and not args.no_lookup:
        d_res, d_off = batches[0]
        res_h = np.empty(n_res, np.uint8)
        off_h = np.empty(n + 1, np.uint64)
        abi.check(L.kgx_memcpy_d2h(res_h.ctypes.data, d_res, res_h.nbytes), "d2h")
        abi.check(L.kgx_memcpy_d2h(off_h.ctypes.data, d_off, off_h.nbytes), "d2h")
        host_path_lookup = host_path_lookup_leg(abi, synth, img, spec, dev, res_h, off_h, params, args.families)

    pool_e2e = pool_lookup = None
    if d.rank == 0 and args.full and not (args.no_pool and args.no_pool_lookup):
        # one replica per rank's device (the other ranks released theirs
        # above): the N-GPU run measures C5 over N devices
        pdevs = pool_devices(dev, n_dev, d.world)
        rep = img_bytes["packed16"] if img.layout == abi.Image.PACKED16 else img_bytes["aos24"]
        hbm_check(abi, pdevs[1:], rep + POOL_HBM, f"an image replica ({rep / GB:.1f} GB) and the C5 pool's "
                                                  f"buffers ({POOL_HBM / GB:.0f} GB)")
        hbm_check(abi, pdevs[:1], POOL_HBM, f"the C5 pool's buffers ({POOL_HBM / GB:.0f} GB)")
        t0 = time.time()
        images = [img] + [img.replicate(dv) for dv in pdevs[1:]]
        t_rep = time.time() - t0
        pin, poff = c5_batch(abi, L, img, spec, args.strong_seq, Ls, args.x_permille)
        if not args.no_pool:
            pool_e2e = pool_e2e_leg(abi, images, pin, poff, params, want)
            pool_e2e["replicate_s"] = round(t_rep, 2)
        if not args.no_pool_lookup:
            pool_lookup = pool_lookup_leg(abi, synth, images, spec, pin, poff, params, args.families)
        for im in images[1:]:
            im.close()
        del pin

    ceiling = None
    if d.rank == 0 and args.full and not args.no_microbench:
        ceiling = {}
        n_reads = int(min(n, 100000) * max(0, Ls - 8) * 1.4)
        for mode, name, useful in ((0, "bucket24", 24), (1, "key8", 8), (2, "sector64", 64),
                                   (3, "rec16", 16), (4, "line64", 64), (5, "line128", 128)):
            ms, reads = ctypes.c_float(), ctypes.c_uint64()
            abi.check(L.kgx_microbench_random_read(ctx.handle, n_reads, mode, ctypes.byref(ms),
                                                   ctypes.byref(reads)), "microbench")  # warm
            abi.check(L.kgx_microbench_random_read(ctx.handle, n_reads, mode, ctypes.byref(ms),
                                                   ctypes.byref(reads)), "microbench")
            rate = reads.value / (ms.value / 1e3)
            ceiling[name] = {"reads_per_s": rate, "useful_GBps": rate * useful / 1e9,
                             "ms": ms.value, "reads": reads.value}
            log(f"[bench] random-read {name}: {rate / 1e9:.2f} G reads/s = "
                f"{rate * useful / 1e9:.0f} GB/s useful")

    cpu = None
    parity = None
    # the CPU port is timed at N=1 only (one host, one baseline; at N>1 the
    # other ranks would wait on rank 0's host copy of the image); the parity
    # check of batch 0 runs on rank 0 at every N
    want_cpu = d.rank == 0 and d.world == 1 and args.full and not args.no_cpu_baseline
    if got0 is not None or want_cpu:
        import oracle
        oracle.build(ref=False)
        t_auto, aff, quota = host_cpus()
        threads = args.cpu_threads or t_auto
        t0 = time.time()
        table = img.download()
        log(f"[bench] image copied to host in {time.time() - t0:.1f}s ({table.nbytes / 1e9:.1f} GB)")
        if got0 is not None:
            parity, _ = parity_check(oracle, table, got0, res0, off0, want, threads, timed_load)
            del got0
            log(f"[bench] parity vs oracle over {parity['sequences']} sequences (want {want}, line index "
                f"{parity['line_index']}): {'equal' if parity['equal'] else 'MISMATCH ' + str(parity['by_output'])}")
        if want_cpu:
            ns = min(args.cpu_sample, n)
            if res0 is None:
                d_res, d_off = batches[0]
                res0 = np.empty(n_res, np.uint8)
                off0 = np.empty(n + 1, np.uint64)
                abi.check(L.kgx_memcpy_d2h(res0.ctypes.data, d_res, res0.nbytes), "d2h")
                abi.check(L.kgx_memcpy_d2h(off0.ctypes.data, d_off, off0.nbytes), "d2h")
            cpu = cpu_baseline(oracle, table, res0[:int(off0[ns])], off0[:ns + 1], threads, args.cpu_seconds, want)
            cpu["affinity_cpus"] = aff
            cpu["cgroup_cpu_quota"] = quota
            log(f"[bench] cpu baseline {cpu['value']:.3e} residues/s on {threads} threads "
                f"(affinity {aff} CPUs, cgroup quota {quota}), P = {cpu['pbar']:.4f}")
        del table

    release()

    if d.rank == 0:
        windows_per_launch = n * max(0, Ls - 8)  # x_permille = 0: every window is probed
        pbar = cpu["pbar"] if cpu else None
        pbar_source = "measured (CPU baseline leg, this run)" if pbar is not None else None
        probe_s = float(np.mean(probe_ms)) / 1e3 if probe_ms else None  # event-timed with --full
        traffic = None
        traffic_source = None
        if args.full and os.path.exists(args.traffic_json):
            try:
                tj = json.load(open(args.traffic_json))
                if (tj.get("n_keys") == n_keys and tj.get("keys_stored") == stored and tj.get("n_seq") == n
                        and tj.get("length") == Ls and tj.get("image_layout", "AOS24") == layout
                        and tj.get("line_index", 0) == timed_load):
                    traffic = tj.get("hbm_bytes_per_launch")
                    traffic_source = (f"not measured in this run: FETCH_SIZE + WRITE_SIZE per probe launch from "
                                      f"profiles/{os.path.basename(args.traffic_json)} "
                                      f"({tj.get('collected', 'an earlier rocprofv3 --pmc run')}), same workload")
                    if pbar is None and tj.get("pbar_measured"):
                        pbar = tj["pbar_measured"]  # the same workload's P measured by an earlier run
                        pbar_source = f"measured earlier on this workload ({os.path.basename(args.traffic_json)})"
            except Exception:
                traffic = None
        if pbar is None:
            # alpha = stored / num_sigs; linear probing, unsuccessful search (an upper bound)
            a = stored / spec.num_sigs
            pbar = 0.5 * (1 + 1 / (1 - a) ** 2)
            pbar_source = "analytic: linear probing, unsuccessful search (upper bound)"
        alg_bytes = windows_per_launch * (24.0 * pbar + 1.0)
        achieved = alg_bytes / probe_s if probe_s else None
        residues_per_step_job = n_global * Ls  # every rank's shard of every step
        value = residues_per_step_job * args.steps / t_max
        if args.strong:
            workload = (f"C5: {n_global} x {Ls}-aa synthetic proteins per step split across {d.world} GPU(s) "
                        f"(residue-balanced shards) vs {n_keys:,}-entry signature image replicated per GPU")
        else:
            workload = (f"C2: {n} x {Ls}-aa synthetic proteins per GPU vs {n_keys:,}-entry signature image "
                        f"({spec.num_sigs:,} buckets, {spec.num_sigs * 24 / 1e9:.1f} GB) resident in HBM")
        line_ceiling = ceiling["line64"] if ceiling else None
        line = {
            "metric": METRIC,
            "value": value,
            "unit": "residues/s",
            "n_gpus": d.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": t_max / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong" if args.strong else "weak",
            "vs_baseline": None,
            "dtype": "u64",
            "data": "synthetic",
            "config": {
                "workload": workload,
                "n_seq_per_gpu": n, "n_seq_per_step": n_global, "seq_len": Ls, "n_keys": n_keys,
                "keys_stored": stored, "stream_entries": n_entries,
                "load_factor": stored / spec.num_sigs,
                "presence_filter_bits": (1 << args.filter_log2) if args.filter_log2 else 0,
                "num_sigs": spec.num_sigs, "parallelism": f"replicas{d.world}",
                "sharding": "one image replica + one contiguous query shard per GPU, no data-path collective",
                "per_rank": per_rank,
                "worker_contexts": len(ctxs), "distinct_batches": len(batches),
                "hits_total": total_hits,
                "score_variant": args.score_variant, "probe_lds_kb": args.probe_lds_kb,
                "probe_persist": args.probe_persist, "probe_stream": args.probe_stream,
                # the score stage alone (HIP events on the context's stream, same
                # untimed pass as the probe time): what a single-context caller pays
                "score_stage_ms": float(np.mean(score_ms)) if score_ms else None,
                "want": want,
                "outputs": WANT_OUTPUTS.get(want, f"want={want}"),
                "canary": ({"ok": all(r["ok"] for r in canary_recs), "digest": canary_recs[0]["digest"][:16],
                            "check": "every rank's canary digest == the CPU oracle's (tests/golden/canary)"}
                           if canary_recs else None),
            },
            "roofline": None if not args.full else {
                "bound": "hbm",
                "achieved": achieved / 1e9,
                "peak": HBM_PEAK / 1e9,
                "unit": "GB/s",
                "frac": achieved / HBM_PEAK,
                "traffic": traffic,
                "traffic_source": traffic_source,
                "kernel": probe_kernel,
                "kernel_ms": probe_s * 1e3,
                "windows_per_launch": windows_per_launch,
                "alg_bytes_per_launch": alg_bytes,
                "pbar": pbar,
                "pbar_source": pbar_source,
                "random_read_ceiling": ceiling,
                "probe_ab": probe_ab,
                # SURVEY §8(d) prices a bucket at the file's 24 B; the PACKED16
                # resident layout moves 16 B per bucket examined
                "image_layout": layout,
                # kgx_image_set_line_index load (0: probes over the reference slots)
                "line_index": timed_load,
                "line_index_lines": line_lines,
                "alg_bytes_per_launch_resident_layout": windows_per_launch * (
                    (16.0 if layout == "PACKED16" else 24.0) * pbar + 1.0),
                # north_star: algorithmic bytes/s (24 P + 1 per window) over the
                # measured random-access bandwidth of the same buffer (useful
                # bytes/s of the cooperative random 64-B line reads the probe does)
                "frac_of_measured_random_access": (
                    achieved / (line_ceiling["useful_GBps"] * 1e9) if line_ceiling else None),
                # the line probe reads >= 1 64-B line per window: windows/s over
                # the random-line rate (a lower bound of the line-rate fraction)
                "frac_of_random_line_rate": (
                    windows_per_launch / probe_s / line_ceiling["reads_per_s"]
                    if line_ceiling and probe_kernel == "probe_line_kernel" else None),
            },
            "cpu_baseline": cpu,
            "parity": parity,
            "line_index_ab": line_ab,
            "pipe_ab": pipe_ab,
            "host_path": host_path,
            "host_path_lookup": host_path_lookup,
            "pool_e2e": pool_e2e,
            "pool_lookup": pool_lookup,
        }
        print(json.dumps(line), flush=True)
    d.close()
    if parity is not None and not parity["equal"]:
        raise SystemExit("parity check failed: the timed configuration's results differ from the oracle's")


if __name__ == "__main__":
    main()
