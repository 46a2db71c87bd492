"""Is this FASTQ file well formed, and how long are its reads: the reference's
validate_fastq.

validate_fastq.cc (:14-107) runs a file through FastqParser with an error
callback that ends the parse, counts the reads that have an id and prints

    valid\\t1                     valid\\t0
    n_seqs\\tN                    n_seqs\\tN
    total_size\\tT                error_message\\t...
    mean\\tM                      error_line\\tL
    stddev\\tS

(the last three lines of a valid file only when N > 0; a file that ends in an
error counts the record in progress if it has an id).  Here the parse is the
library's on the device (abi.Context.fq_parse in strict mode,
csrc/kgx_fq_parse.hip): the file is streamed in blocks, what a
block's parse did not consume is carried in front of the next, and only the two
offset arrays come back.  The sums over the lengths are the reference's, in
double and in record order, on the host.

    python -m close_kmers_amd.validate_fastq FASTQ|- [--device N] [--data DATA_DIR] [--block-bytes N]

Plain text only, as the reference; "-" reads stdin.  The reference's "Error
found: ..." line goes to stderr and the exit status stays 0.
"""
from __future__ import annotations

import argparse
import math
import sys

BLOCK_BYTES = 32 << 20


def report(lengths, error) -> str:
    """The tool's stdout: lengths of the reads that have an id, in record
    order; error None or (message, line)."""
    sizes = [int(x) for x in lengths]
    n = len(sizes)
    if error is not None:
        return f"valid\t0\nn_seqs\t{n}\nerror_message\t{error[0]}\nerror_line\t{error[1]}\n"
    out = f"valid\t1\nn_seqs\t{n}\n"
    if n:
        total = sum(sizes)
        mean = float(total) / float(n)
        stddev = 0.0
        if n > 1:
            accum = 0.0
            for s in sizes:
                d = float(s)
                accum += (d - mean) * (d - mean)
            stddev = math.sqrt(accum / (float(n) - 1.0))
        out += "total_size\t%d\nmean\t%.2f\nstddev\t%.2f\n" % (total, mean, stddev)
    return out


def validate(ctx, blocks):
    """Stream blocks of FASTQ bytes through ctx: (lengths of the reads with an
    id, None or (message, line, id))."""
    import numpy as np

    from . import abi
    lengths = []
    lines = 0  # newlines consumed by the earlier parses

    def parse(text: bytes, flags: int):
        nonlocal lines
        r = ctx.fq_parse(text, flags)
        h = ctx.fq_reads_to_host(r, ("read_offsets", "id_offsets"))
        keep = np.diff(h["id_offsets"].astype(np.int64)) > 0
        lengths.append(np.diff(h["read_offsets"].astype(np.int64))[keep])
        error = None
        if r.error:
            rid = b""
            if r.n_reads:
                a, b = (int(x) for x in h["id_offsets"][-2:])
                ids = np.zeros(b - a, np.uint8)
                if b > a:
                    abi.check(abi.lib().kgx_memcpy_d2h(ids.ctypes.data, r.ids + a, b - a), "d2h")
                rid = ids.tobytes()
            error = (r.error_text(), 1 + lines + r.error_newlines, rid.decode("latin-1"))
        lines += r.newlines
        return r.consumed, error

    tail, error = b"", None
    for b in blocks:
        text = tail + b if tail else b
        consumed, error = parse(text, abi.FQ_STRICT)
        if error:
            break
        tail = text[consumed:]
    if error is None and tail:
        _, error = parse(tail, abi.FQ_STRICT | abi.FQ_FINISHED)
    all_lengths = np.concatenate(lengths) if lengths else np.zeros(0, np.int64)
    return all_lengths, error


def stream_blocks(f, block_bytes: int = BLOCK_BYTES):
    while True:
        b = f.read(block_bytes)
        if not b:
            return
        yield b


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.validate_fastq",
                                 description="Check a FASTQ file and report its reads' lengths.")
    ap.add_argument("fastq", metavar="FASTQ", help="fastq file input (plain text), or - for stdin")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--data", metavar="DATA_DIR", help="kmer data directory for the context's image (default: none)")
    ap.add_argument("--block-bytes", type=int, default=BLOCK_BYTES, help="bytes of text per device pass")
    a = ap.parse_args(argv)
    if a.block_bytes < 1:
        ap.error("--block-bytes must be positive")
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import abi
    from .fastq_to_protein import placeholder_image
    f = sys.stdin.buffer if a.fastq == "-" else open(a.fastq, "rb")
    try:
        img = abi.Image.open(a.data, a.device) if a.data else placeholder_image(abi, a.device)
        with img, abi.Context(img) as ctx:
            lengths, error = validate(ctx, stream_blocks(f, a.block_bytes))
    finally:
        if a.fastq != "-":
            f.close()
    # bytes out as they came in: a bad data character or an id may be any byte
    if error:
        sys.stderr.buffer.write(f"Error found: {error[0]} at line {error[1]} id='{error[2]}'\n".encode("latin-1"))
        sys.stderr.flush()
    sys.stdout.buffer.write(report(lengths, error[:2] if error else None).encode("latin-1"))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
