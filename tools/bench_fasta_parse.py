#!/usr/bin/env python3
"""The FASTA parser on the device against the handlers' host
framing, on the same box in one process.

Input: seeded protein FASTA in 60-column lines (synth.make_queries over the
image's own sources, so the lookups hit), --length residues each (default 300),
at --n-seqs proteins (default 100,000, C2's shape, and 1,000,000).  Per size
one warm-up pass of every leg, then --reps timed passes with the legs
alternating:

  (a) kgx_fa_parse (KGX_FA_FINISHED) from the text in host memory: wall clock,
      and the upload and parse event times;
  (b) kgx::parse_fasta_body_flat on one host thread (tools/fasta_parse_host.cpp,
      built into tools/_build against libkgx.so): wall clock of the parse;
  (c) text -> calls: kgx_fa_parse + kgx_run_device + collect (Context.
      run_parsed) against (b)'s parse + kgx_process_batch, both with
      KGX_WANT_CALLS; the two must return the same call offsets.

One JSON line on stdout; --out FILE also writes it there
(profiles/fa_parse_bench.json).
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "fasta_parse_host.cpp")
OUT = os.path.join(HERE, "_build", "fasta_parse_host.so")


def host_parser(kbuild):
    """tools/_build/fasta_parse_host.so, built when stale."""
    deps = [SRC, kbuild.LIB, os.path.join(kbuild.CSRC, "kgx_handlers.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        cmd = [kbuild.HIPCC, "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "hip", f"--offload-arch={kbuild.ARCH}",
               f"-I{kbuild.INCLUDE}", f"-I{kbuild.CSRC}", SRC, "-o", OUT, f"-L{kbuild.PKG}", "-lkgx",
               f"-Wl,-rpath,{kbuild.PKG}"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError(r.stdout + r.stderr)
    L = ctypes.CDLL(OUT)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    L.fph_parse.argtypes, L.fph_parse.restype = [vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_double)], vp
    for name, res in (("fph_size", u64), ("fph_residues", vp), ("fph_n_residues", u64), ("fph_offsets", vp),
                      ("fph_free", None)):
        getattr(L, name).argtypes, getattr(L, name).restype = [vp], res
    return L


def fasta_text(res: np.ndarray, n: int, length: int) -> np.ndarray:
    """>pK, then the K-th sequence in 60-column lines."""
    rows = res.reshape(n, length)
    lines = [rows[:, k:k + 60] for k in range(0, length, 60)]
    nl = np.full((n, 1), 10, np.uint8)
    body = np.concatenate([np.concatenate([ln, nl], axis=1) for ln in lines], axis=1)
    out = bytearray()
    for k in range(n):
        out += b">p%d\n" % k
        out += body[k].tobytes()
    return np.frombuffer(bytes(out), np.uint8)


def leg_device_parse(abi, ctx, text):
    r = abi.FaSeqs()
    t0 = time.perf_counter()
    abi.check(abi.lib().kgx_fa_parse(ctx.handle, text.ctypes.data, text.nbytes, abi.FA_FINISHED, ctypes.byref(r)),
              "kgx_fa_parse")
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "upload_ms": r.upload_ms, "parse_ms": r.parse_ms}, r


def leg_host_parse(H, text):
    ms = ctypes.c_double()
    t0 = time.perf_counter()
    h = H.fph_parse(text.ctypes.data, text.nbytes, ctypes.byref(ms))
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "parse_ms": ms.value}, h


def leg_device_calls(abi, ctx, text, prm, want):
    t0 = time.perf_counter()
    d, r = leg_device_parse(abi, ctx, text)
    got = ctx.run_parsed(r, prm, want=want)
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "upload_ms": d["upload_ms"], "parse_ms": d["parse_ms"]}, got


def leg_host_calls(abi, ctx, H, text, prm, want):
    t0 = time.perf_counter()
    p, h = leg_host_parse(H, text)
    try:
        n, nr = H.fph_size(h), H.fph_n_residues(h)
        res = np.ctypeslib.as_array(ctypes.cast(H.fph_residues(h), ctypes.POINTER(ctypes.c_uint8)), (max(nr, 1),))[:nr]
        off = np.ctypeslib.as_array(ctypes.cast(H.fph_offsets(h), ctypes.POINTER(ctypes.c_uint64)), (n + 1,))
        got = ctx.process_batch(res, off, prm, want=want)
    finally:
        H.fph_free(h)
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "parse_ms": p["parse_ms"]}, got


def summary(runs, text_bytes):
    out = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    out["all"] = runs
    out["parse_gb_per_s"] = text_bytes / out["parse_ms"] / 1e6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-seqs", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--length", type=int, default=300)
    ap.add_argument("--n-keys", type=float, default=2e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON to this file")
    a = ap.parse_args()
    from close_kmers_amd import abi, build, synth
    build.build()
    H = host_parser(build)
    spec = synth.ImageSpec(int(a.n_keys))
    img, _ = abi.Image.synthetic(spec.n_keys, spec.num_sigs)
    prm, want = abi.Params(5, 200, 0, 0), abi.WANT_CALLS
    result = {"metric": "fa_parse_gb_per_s", "unit": "GB/s", "length": a.length, "reps": a.reps, "n_keys": spec.n_keys,
              "sizes": []}
    with img, abi.Context(img) as ctx:
        for n in a.n_seqs:
            res, _ = synth.make_queries(spec, n, a.length)
            text = fasta_text(res, n, a.length)
            legs = {"device_parse": [], "host_parse": [], "device_text_to_calls": [], "host_text_to_calls": []}
            for rep in range(a.reps + 1):  # the first pass warms every leg
                d, r = leg_device_parse(abi, ctx, text)
                assert (r.n_seqs, r.n_residues, r.error) == (n, n * a.length, 0)
                p, h = leg_host_parse(H, text)
                assert H.fph_size(h) == n and H.fph_n_residues(h) == n * a.length
                H.fph_free(h)
                dc, got = leg_device_calls(abi, ctx, text, prm, want)
                hc, ref = leg_host_calls(abi, ctx, H, text, prm, want)
                assert np.array_equal(got.call_offsets, ref.call_offsets) and int(ref.call_offsets[-1]) > 0
                if rep:
                    for k, v in (("device_parse", d), ("host_parse", p), ("device_text_to_calls", dc),
                                 ("host_text_to_calls", hc)):
                        legs[k].append(v)
            size = {"n_seqs": n, "text_bytes": int(text.nbytes), "calls": int(ref.call_offsets[-1])}
            size.update({k: summary(v, text.nbytes) for k, v in legs.items()})
            size["parse_speedup"] = size["host_parse"]["parse_ms"] / size["device_parse"]["parse_ms"]
            size["text_to_calls_speedup"] = size["host_text_to_calls"]["wall_ms"] / size["device_text_to_calls"]["wall_ms"]
            result["sizes"].append(size)
            print(json.dumps(size), file=sys.stderr, flush=True)
    result["value"] = result["sizes"][-1]["device_parse"]["parse_gb_per_s"]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
