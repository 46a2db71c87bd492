"""Is this FASTA file well formed, and how long are its sequences: the
reference's validate_fasta.

validate_fasta.cc (:12-82) runs a file through FastaParser with an error
callback that ends the parse, counts the records that have an id and prints
what validate_fastq prints (validate_fastq.report: valid, n_seqs and, for a
valid file with sequences, total_size, mean and stddev; else error_message and
error_line).  A file that ends in an error counts the record in progress if it
has an id.  Here the parse is the library's on the device
(abi.Context.fa_parse in strict mode, csrc/kgx_fa_parse.hip):
the file is streamed in blocks, what a block's parse did not consume is
carried in front of the next, the last parse is the tail's as the end of the
input, and only the two offset arrays come back (and the last id on an error).

    python -m close_kmers_amd.validate_fasta FASTA|- [--device N] [--data DATA_DIR] [--block-bytes N]

Plain text only, as the reference; "-" reads stdin.  The reference's "Error
found: ..." line goes to stderr and the exit status stays 0.
"""
from __future__ import annotations

import argparse
import sys

from .validate_fastq import BLOCK_BYTES, report, stream_blocks


def validate(ctx, blocks):
    """Stream blocks of FASTA bytes through ctx: (lengths of the records with
    an id, None or (message, line, id))."""
    import numpy as np

    from . import abi
    lengths = []
    lines = 0  # newlines consumed by the earlier parses

    def parse(text: bytes, flags: int):
        nonlocal lines
        r = ctx.fa_parse(text, flags)
        h = ctx.fa_seqs_to_host(r, ("seq_offsets", "id_offsets"))
        keep = np.diff(h["id_offsets"].astype(np.int64)) > 0
        lengths.append(np.diff(h["seq_offsets"].astype(np.int64))[keep])
        error = None
        if r.error:
            rid = b""
            if r.n_seqs:
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
        consumed, error = parse(text, abi.FA_STRICT)
        if error:
            break
        tail = text[consumed:]
    if error is None:
        _, error = parse(tail, abi.FA_STRICT | abi.FA_FINISHED)
    all_lengths = np.concatenate(lengths) if lengths else np.zeros(0, np.int64)
    return all_lengths, error


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.validate_fasta",
                                 description="Check a FASTA file and report its sequences' lengths.")
    ap.add_argument("fasta", metavar="FASTA", help="fasta file input (plain text), or - for stdin")
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
    f = sys.stdin.buffer if a.fasta == "-" else open(a.fasta, "rb")
    try:
        img = abi.Image.open(a.data, a.device) if a.data else placeholder_image(abi, a.device)
        with img, abi.Context(img) as ctx:
            lengths, error = validate(ctx, stream_blocks(f, a.block_bytes))
    finally:
        if a.fasta != "-":
            f.close()
    # bytes out as they came in: a bad character or an id may be any byte
    if error:
        sys.stderr.buffer.write(f"Error found: {error[0]} at line {error[1]} id='{error[2]}'\n".encode("latin-1"))
        sys.stderr.flush()
    sys.stdout.buffer.write(report(lengths, error[:2] if error else None).encode("latin-1"))
    sys.stdout.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
