#!/usr/bin/env python3
"""fastq_to_protein on the device: FASTQ text in host memory
to FASTA text in host memory.

Reads: C4's (uniform ACGT, 150 bp, seed 0x5EED0004, the text made as
tools/bench_fq.py makes it), at --n-reads (default 1M and 10M).  Per size:
one warm-up pass over the first --warm-reads reads, then --reps timed passes
of the whole text through one kgx_f2p handle in --block-mb blocks; the median
pass gives reads/s, its stage times (kgx_f2p_get_stats), the output bytes and
the writer's bytes per second of stream time.

Two baselines on the same box:
  (a) today's alternative: kgx_fq_fragments with residues written, the
      arrays copied to the host, the records formatted there on one thread.
      That path has no token index, so it writes 0 in its place: a lower
      bound of its cost.  Python formats about a million records a second, so
      it runs over --host-reads reads and its rate is per read.
  (b) a device-to-device copy of as many bytes as a part's text: the floor
      for the writer.
--parse-device 0, 1 or both runs the sizes with the context's option
"fq_parse_device" at that value (both: 0 first, then 1, same
process, same text, same warm-up and reps); with more than one setting the
result holds "parse_device": {setting: sizes}.  Every size then also reports
parse_gb_per_s, the FASTQ bytes per second of parse_ms (at 1: the parse
kernels' stream time), and baseline_d2d_part_text is the device-to-device copy
of one part's FASTQ text, the floor for those kernels.  --validate adds the
validate_fastq leg: the same text in host memory through kgx_fq_parse in
strict mode in --block-mb blocks, the unconsumed tail fed again, the offset
arrays downloaded and the lengths summed.  --out FILE also writes the JSON
there.
One JSON line on stdout.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_fq import fastq_text_fast  # noqa: E402

STAGES = ("parse_ms", "upload_ms", "index_ms", "sizes_ms", "write_ms", "download_ms")


def one_pass(abi, h, text: np.ndarray, block: int) -> dict:
    """The whole text through the handle; the output is touched, not copied."""
    L = abi.lib()
    t, n = ctypes.c_void_p(), ctypes.c_uint64()
    base, size, out_bytes = text.ctypes.data, text.nbytes, 0
    t0 = time.perf_counter()
    for at in range(0, size, block):
        m = min(block, size - at)
        abi.check(L.kgx_f2p_process(h.handle, ctypes.cast(base + at, ctypes.c_char_p), m, int(at + m == size),
                                    ctypes.byref(t), ctypes.byref(n)), "kgx_f2p_process")
        out_bytes += n.value
    wall = time.perf_counter() - t0
    st = h.stats()
    assert st["text_bytes"] == out_bytes and st["error_line"] == 0
    return dict(st, wall_s=wall)


def validate_pass(abi, ctx, text: np.ndarray, block: int) -> dict:
    """validate_fastq's work over text in host memory: strict parses of
    blocks, each starting where the last one's consumed bytes end."""
    L = abi.lib()
    base, size, at = text.ctypes.data, text.nbytes, 0
    n_seqs = total = 0
    parse_ms = upload_ms = 0.0
    t0 = time.perf_counter()
    while at < size:
        m = min(block, size - at)
        last = at + m == size
        r = abi.FqReads()
        abi.check(L.kgx_fq_parse(ctx.handle, base + at, m, abi.FQ_STRICT | (abi.FQ_FINISHED if last else 0),
                                 ctypes.byref(r)), "kgx_fq_parse")
        assert r.error == 0 and r.consumed > 0
        h = ctx.fq_reads_to_host(r, ("read_offsets", "id_offsets"))
        keep = np.diff(h["id_offsets"].astype(np.int64)) > 0
        lengths = np.diff(h["read_offsets"].astype(np.int64))[keep]
        n_seqs += len(lengths)
        total += int(lengths.sum())
        parse_ms += r.parse_ms
        upload_ms += r.upload_ms
        at += r.consumed
    return {"wall_s": time.perf_counter() - t0, "n_seqs": n_seqs, "total_size": total, "parse_ms": parse_ms,
            "upload_ms": upload_ms}


def host_baseline(abi, ctx, bases: np.ndarray, length: int, n: int) -> dict:
    """(a): fragments with residues -> host arrays -> text on one thread."""
    off = np.arange(n + 1, dtype=np.uint64) * length
    ctx.set_option("fq_residues", 1)
    ctx.fragments_to_host(ctx.fq_fragments(bases[:n * length], off))  # warm: the buffers exist
    t0 = time.perf_counter()
    f = ctx.fq_fragments(bases[:n * length], off)
    h = ctx.fragments_to_host(f)
    t1 = time.perf_counter()
    res, o = h["residues"].tobytes(), h["offsets"].tolist()
    out = [b">r%09d:%d:0\n%s\n" % (r, fr, res[a:b])
           for r, fr, a, b in zip(h["read"].tolist(), h["frame"].tolist(), o[:-1], o[1:])]
    text = b"".join(out)
    t2 = time.perf_counter()
    return {"reads": n, "fragments": int(f.n_fragments), "text_bytes": len(text), "device_and_copy_s": t1 - t0,
            "format_s": t2 - t1, "reads_per_s": n / (t2 - t0)}


def d2d_baseline(abi, ctx, nbytes: int, reps: int = 20) -> dict:
    """(b): a device-to-device copy of nbytes on the context's stream, the
    median of reps (HIP events; the runtime the library already loaded)."""
    hip = ctypes.CDLL("libamdhip64.so")
    L = abi.lib()

    def ok(rc, what):
        if rc:
            raise RuntimeError(f"{what}: hip error {rc}")
    src, dst = ctypes.c_void_p(), ctypes.c_void_p()
    abi.check(L.kgx_device_alloc(0, nbytes, ctypes.byref(src)), "alloc")
    abi.check(L.kgx_device_alloc(0, nbytes, ctypes.byref(dst)), "alloc")
    fill = np.random.default_rng(1).integers(0, 255, nbytes, dtype=np.uint8)
    abi.check(L.kgx_memcpy_h2d(src, fill.ctypes.data, nbytes), "h2d")
    stream = ctypes.c_void_p(ctx.stream)
    e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
    ok(hip.hipEventCreate(ctypes.byref(e0)), "hipEventCreate")
    ok(hip.hipEventCreate(ctypes.byref(e1)), "hipEventCreate")
    ms = []
    for i in range(5 + reps):
        ok(hip.hipEventRecord(e0, stream), "hipEventRecord")
        ok(hip.hipMemcpyAsync(dst, src, ctypes.c_size_t(nbytes), 3, stream), "hipMemcpyAsync")  # device to device
        ok(hip.hipEventRecord(e1, stream), "hipEventRecord")
        ok(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        t = ctypes.c_float()
        ok(hip.hipEventElapsedTime(ctypes.byref(t), e0, e1), "hipEventElapsedTime")
        if i >= 5:
            ms.append(t.value)
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    L.kgx_device_free(src)
    L.kgx_device_free(dst)
    m = statistics.median(ms)
    return {"bytes": nbytes, "ms": m, "gb_per_s": nbytes / m / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-reads", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm-reads", type=int, default=200_000)
    ap.add_argument("--block-mb", type=int, default=64)
    ap.add_argument("--part-bytes", type=int, default=0)
    ap.add_argument("--host-reads", type=int, default=200_000)
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--parse-device", choices=("0", "1", "both"), default="0")
    ap.add_argument("--validate", action="store_true", help="add the validate_fastq leg")
    ap.add_argument("--out", help="also write the JSON to this file")
    a = ap.parse_args()
    from close_kmers_amd import abi, build, fastq_to_protein
    build.build()
    n_max, Lr = max(a.n_reads), a.length
    rng = np.random.default_rng(0x5EED0004)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_max * Lr, dtype=np.uint8)]
    result = {"metric": "fastq_to_protein_reads_per_s", "unit": "reads/s", "length": Lr, "reps": a.reps,
              "block_mb": a.block_mb, "part_bytes": a.part_bytes or 32 << 20, "sizes": []}
    with fastq_to_protein.placeholder_image(abi) as img, abi.Context(img) as ctx:
        part_text = 0
        settings = (0, 1) if a.parse_device == "both" else (int(a.parse_device),)
        by_setting = {v: [] for v in settings}
        legs = []
        for n in a.n_reads:
            text = np.frombuffer(fastq_text_fast(bases, Lr, 0, n), np.uint8)
            for v in settings:
                ctx.set_option("fq_parse_device", v)
                with abi.FastqToProtein(ctx, a.part_bytes) as h:
                    w = min(n, a.warm_reads)
                    one_pass(abi, h, text[:w * (text.nbytes // n)], a.block_mb << 20)
                    runs = sorted((one_pass(abi, h, text, a.block_mb << 20) for _ in range(a.reps)),
                                  key=lambda r: r["wall_s"])
                med = runs[len(runs) // 2]
                part_text = med["text_bytes"] // max(1, med["parts"])
                by_setting[v].append({
                    "reads": n, "fastq_bytes": int(text.nbytes), "reads_per_s": n / med["wall_s"],
                    "wall_s": med["wall_s"], "wall_s_all": [r["wall_s"] for r in runs],
                    "fragments": med["fragments"], "text_bytes": med["text_bytes"], "parts": med["parts"],
                    "stage_ms": {k: med[k] for k in STAGES},
                    "stage_ms_all": [{k: r[k] for k in STAGES} for r in runs],
                    "device_ms": sum(med[k] for k in STAGES[1:]),
                    "parse_gb_per_s": text.nbytes / med["parse_ms"] / 1e6,
                    "writer_gb_per_s": med["text_bytes"] / med["write_ms"] / 1e6,
                    "download_gb_per_s": med["text_bytes"] / med["download_ms"] / 1e6})
                print(json.dumps(dict(by_setting[v][-1], fq_parse_device=v)), file=sys.stderr, flush=True)
            ctx.set_option("fq_parse_device", 0)
            if a.validate:
                w = min(n, a.warm_reads)
                validate_pass(abi, ctx, text[:w * (text.nbytes // n)], a.block_mb << 20)
                runs = sorted((validate_pass(abi, ctx, text, a.block_mb << 20) for _ in range(a.reps)),
                              key=lambda r: r["wall_s"])
                med = runs[len(runs) // 2]
                assert med["n_seqs"] == n and med["total_size"] == n * Lr
                legs.append(dict(med, reads=n, fastq_bytes=int(text.nbytes), wall_s_all=[r["wall_s"] for r in runs],
                                 reads_per_s=n / med["wall_s"], parse_gb_per_s=text.nbytes / med["parse_ms"] / 1e6,
                                 host_gb_per_s=text.nbytes / med["wall_s"] / 1e9))
                print(json.dumps(dict(legs[-1], leg="validate_fastq")), file=sys.stderr, flush=True)
            del text
        result["sizes"] = by_setting[settings[-1]] if len(settings) == 1 else by_setting[0]
        if len(settings) > 1:
            result["parse_device"] = {str(v): by_setting[v] for v in settings}
        if a.validate:
            result["validate_fastq"] = legs
        result["value"] = result["sizes"][-1]["reads_per_s"]
        if not a.no_baselines:
            result["baseline_host_format"] = host_baseline(abi, ctx, bases, Lr, min(n_max, a.host_reads))
            result["baseline_d2d_copy"] = d2d_baseline(abi, ctx, part_text)
            result["speedup_over_host_format"] = result["value"] / result["baseline_host_format"]["reads_per_s"]
            result["writer_fraction_of_d2d"] = result["sizes"][-1]["writer_gb_per_s"] / \
                result["baseline_d2d_copy"]["gb_per_s"]
        if len(settings) > 1 or a.validate:
            result["baseline_d2d_part_text"] = d2d_baseline(abi, ctx, min(result["part_bytes"],
                                                                       result["sizes"][-1]["fastq_bytes"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
