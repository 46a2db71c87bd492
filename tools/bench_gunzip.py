#!/usr/bin/env python3
"""Inflating BGZF FASTQ: GB/s of *output* for

  (a) inflate_members_kernel alone, by events (kgx_gunzip_device);
  (b) kgx_gunzip host to host on the device (upload, kernel, download; the
      split comes from its statistics);
  (c) kgx_gunzip with option gunzip_device 0: the same decoder on up to 16
      host threads;
  (d) zlib.decompress member by member on one thread: the library and the
      threading the reference uses per request.

The text is bench_fq's (fastq_text_fast), compressed here by Python's zlib at
chunk 65,280, level 6 and level 1; the compression time is reported and is
part of no figure.  Every figure is run --reps times in this process and every
run is reported.  The verdict line applies the rule for the default of
"gunzip_device": 1 only if every run of (b) beats 16 x the best run of (d)
by more than the spread of (b)'s own runs.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def bgzf_member(part: bytes, level: int) -> bytes:
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9)
    raw = c.compress(part) + c.flush()
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 0x42, 0x43, 2, len(raw) + 25)
    return head + raw + struct.pack("<II", zlib.crc32(part), len(part))


def bgzf_bytes(data: bytes, level: int = 6, chunk: int = 65280, threads: int = 16) -> bytes:
    """`data` as blocked gzip members of `chunk` bytes (zlib releases the GIL: threads)"""
    parts = [data[i:i + chunk] for i in range(0, len(data), chunk)]
    with ThreadPoolExecutor(threads) as ex:
        members = list(ex.map(lambda p: bgzf_member(p, level), parts, chunksize=64))
    return b"".join(members) + BGZF_EOF


def member_rows(gz: bytes):
    """(in_off, out_off, in_len, out_len, crc, 0) per member"""
    rows, at, out = [], 0, 0
    while at < len(gz):
        total = int.from_bytes(gz[at + 16:at + 18], "little") + 1
        crc, isize = struct.unpack_from("<II", gz, at + total - 8)
        rows.append((at + 18, out, total - 26, isize, crc, 0))
        out += isize
        at += total
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-reads", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_bench.json"))
    args = ap.parse_args()

    from bench_fq import fastq_text_fast
    rng = np.random.default_rng(0x5EED0004)
    bases = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, args.n_reads * args.length, dtype=np.uint8)]
    text = fastq_text_fast(bases, args.length, 0, args.n_reads)
    del bases
    bodies = {}
    for level in (6, 1):
        t0 = time.perf_counter()
        bodies[f"level{level}"] = bgzf_bytes(text, level)
        print(f"[bench_gunzip] level {level}: {len(text) / 1e6:.0f} MB -> {len(bodies[f'level{level}']) / 1e6:.0f} MB "
              f"in {time.perf_counter() - t0:.1f}s (not timed)", file=sys.stderr, flush=True)

    from close_kmers_amd import abi, synth
    L = abi.lib()
    spec = synth.ImageSpec(20000)
    img, _ = abi.Image.synthetic(spec.n_keys, spec.num_sigs)
    ctx = abi.Context(img)
    gb = len(text) / 1e9
    h_out = ctypes.c_void_p()
    abi.check(L.kgx_host_alloc(len(text) + 64, ctypes.byref(h_out)), "kgx_host_alloc")
    result = {"note": "GB/s of inflated output; FASTQ text of bench_fq.fastq_text_fast as BGZF, chunk 65,280",
              "n_reads": args.n_reads, "read_len": args.length, "text_bytes": len(text), "reps": args.reps,
              "bodies": {}}
    for name, gz in bodies.items():
        rows = member_rows(gz)
        members = np.array(rows, dtype=abi.GZ_MEMBER_DTYPE)
        r = {"compressed_bytes": len(gz), "members": len(rows)}
        # (a) the kernel alone
        d_gz, d_out = ctypes.c_void_p(), ctypes.c_void_p()
        abi.check(L.kgx_device_alloc(0, len(gz), ctypes.byref(d_gz)), "alloc")
        abi.check(L.kgx_device_alloc(0, len(text) + 64, ctypes.byref(d_out)), "alloc")
        abi.check(L.kgx_memcpy_h2d(d_gz, gz, len(gz)), "h2d")
        ms = []
        for i in range(args.reps + 1):
            rc, status, _, k_ms = abi.gunzip_device(ctx, d_gz.value, members, d_out.value)
            abi.check(rc, "kgx_gunzip_device")
            if i:
                ms.append(k_ms)
        r["a_kernel_ms"] = ms
        r["a_kernel_GBps"] = [gb / (m / 1e3) for m in ms]
        L.kgx_device_free(d_gz)
        L.kgx_device_free(d_out)

        # (b), (c) host to host
        def host_to_host():
            n, used, st = ctypes.c_uint64(), ctypes.c_uint64(), abi.GunzipStats()
            t0 = time.perf_counter()
            abi.check(L.kgx_gunzip(ctx.handle, gz, len(gz), 1, h_out, len(text) + 64, ctypes.byref(n),
                                   ctypes.byref(used), ctypes.byref(st)), "kgx_gunzip")
            dt = time.perf_counter() - t0
            assert n.value == len(text) and used.value == len(gz)
            return dt, st.as_dict()
        for key, device in (("b_device", 1), ("c_host16", 0)):
            ctx.set_option("gunzip_device", device)
            host_to_host()  # warm: buffer growth
            assert zlib.crc32(ctypes.string_at(h_out, len(text))) == zlib.crc32(text)
            runs = [host_to_host() for _ in range(args.reps)]
            r[key + "_ms"] = [dt * 1e3 for dt, _ in runs]
            r[key + "_GBps"] = [gb / dt for dt, _ in runs]
            if device:
                r["b_split_ms"] = [{k: st[k] for k in ("upload_ms", "kernel_ms", "download_ms")} for _, st in runs]
        # (d) zlib, one thread, member by member
        raws = [gz[a:a + n] for a, _, n, _, _, _ in rows]
        d = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            total = 0
            for raw in raws:
                total += len(zlib.decompress(raw, -15))
            d.append(time.perf_counter() - t0)
            assert total == len(text)
        r["d_zlib1_ms"] = [x * 1e3 for x in d]
        r["d_zlib1_GBps"] = [gb / x for x in d]
        b, z = r["b_device_GBps"], max(r["d_zlib1_GBps"])
        r["rule"] = {"b_min": min(b), "b_spread": max(b) - min(b), "zlib_x16": 16 * z,
                     "device_default": bool(min(b) - 16 * z > max(b) - min(b))}
        result["bodies"][name] = r
        print(f"[bench_gunzip] {name}: kernel {max(r['a_kernel_GBps']):.1f} GB/s, host-to-host "
              f"{min(b):.2f}-{max(b):.2f} GB/s, 16 host threads {max(r['c_host16_GBps']):.2f} GB/s, "
              f"16 x zlib {16 * z:.2f} GB/s", file=sys.stderr, flush=True)
    result["gunzip_device_default"] = int(all(r["rule"]["device_default"] for r in result["bodies"].values()))
    L.kgx_host_free(h_out)
    ctx.close()
    img.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({"metric": "kgx_gunzip host-to-host GB/s of output (BGZF level 6)",
                      "value": min(result["bodies"]["level6"]["b_device_GBps"]), "unit": "GB/s",
                      "gunzip_device_default": result["gunzip_device_default"]}), flush=True)


if __name__ == "__main__":
    main()
