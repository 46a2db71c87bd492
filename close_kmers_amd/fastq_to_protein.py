"""Reads to six-frame protein FASTA: the reference's fastq_to_protein.

fastq_to_protein.cc (:14-58) reads a FASTQ file and writes, for every read
with an id and each frame 1, 2, 3, -1, -2, -3, every token of the code-11
translation split at '*' that is longer than 10 residues as

    >ID:FRAME:INDEX
    TOKEN

INDEX counting all the frame's tokens from 1.  Here the parse is the
library's (the tool's own rule: the first parse error ends the file, the
record in progress still goes out), and the token indices, the record layout
and the text are made on the device (abi.FastqToProtein, csrc/kgx_fq.hip,
DESIGN.md §8.11); only finished text comes back.

    python -m close_kmers_amd.fastq_to_protein FASTQ [-o FILE] [--device N] [--data DATA_DIR] \\
        [--part-bytes N]

The file is streamed in blocks and the output is never held whole.  A gzip
or BGZF file is inflated by the library (the reference reads plain files
only).  A parse error is reported on stderr as the reference words it and the
exit status stays 0, as the reference's.  The tool needs no k-mer image;
without --data its context stands on a one-key image built in memory.
"""
from __future__ import annotations

import argparse
import sys

BLOCK_BYTES = 16 << 20


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.fastq_to_protein",
                                 description="Translate FASTQ reads in six frames to protein FASTA.")
    ap.add_argument("fastq", metavar="FASTQ", help="fastq file input (plain, gzip or BGZF)")
    ap.add_argument("-o", "--output-file", dest="output", help="output file (default: stdout)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--data", metavar="DATA_DIR", help="kmer data directory for the context's image (default: none)")
    ap.add_argument("--part-bytes", type=int, default=0,
                    help="FASTQ bytes per device pass (0: the library's default, 32 MB)")
    a = ap.parse_args(argv)
    if a.part_bytes < 0:
        ap.error("--part-bytes must not be negative")
    return a


def placeholder_image(abi, device: int = 0):
    """An image of one key: a context needs one, the translation reads none."""
    from . import synth
    img, _ = abi.Image.build([0], [0], [-1], [0], [1.0], synth.builder_num_sigs(1), device)
    return img


def translate(ctx, blocks, write, part_bytes: int = 0):
    """Stream blocks of FASTQ bytes through ctx, hand each block's text to
    write(); returns (stats, the parse error's report or "")."""
    from . import abi
    with abi.FastqToProtein(ctx, part_bytes) as h:
        last = None
        for b in blocks:
            if last is not None:
                text = h.process(last, False)
                if text:
                    write(text)
            last = b
        text = h.process(last if last is not None else b"", True)
        if text:
            write(text)
        return h.stats(), h.error()


def file_blocks(path: str, block_bytes: int = BLOCK_BYTES):
    with open(path, "rb") as f:
        while True:
            b = f.read(block_bytes)
            if not b:
                return
            yield b


def main(argv=None) -> int:
    a = parse_args(argv)
    from . import abi
    out = open(a.output, "wb") if a.output else sys.stdout.buffer
    try:
        img = abi.Image.open(a.data, a.device) if a.data else placeholder_image(abi, a.device)
        with img, abi.Context(img) as ctx:
            _, err = translate(ctx, file_blocks(a.fastq), out.write, a.part_bytes)
        out.flush()
    finally:
        if a.output:
            out.close()
    if err:
        print(err, file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
