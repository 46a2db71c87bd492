"""FASTA files read through the device parser (abi.Context.fa_parse,
csrc/kgx_fa_parse.hip): the records the reference's
FastaParser hands over, parse_complete's last one included -- the id runs to
the first blank ("> x" has an empty id), '\\r' is skipped, a byte the parser
reports is dropped.
"""
from __future__ import annotations

from .validate_fastq import BLOCK_BYTES, stream_blocks


def records_of(ctx, r) -> list[tuple[bytes, bytes]]:
    """[(id, sequence)] of a FaSeqs, downloaded."""
    h = ctx.fa_seqs_to_host(r)
    ids, res = h["ids"].tobytes(), h["residues"].tobytes()
    io, so = h["id_offsets"].tolist(), h["seq_offsets"].tolist()
    return [(ids[io[k]:io[k + 1]], res[so[k]:so[k + 1]]) for k in range(r.n_seqs)]


def read_records(ctx, path, block_bytes: int = BLOCK_BYTES) -> list[tuple[bytes, bytes]]:
    """The records of the FASTA file at path: lenient parses of block_bytes of
    text each, what a parse did not consume carried in front of the next block,
    the file's last part parsed as the end of the input."""
    from . import abi
    records: list[tuple[bytes, bytes]] = []
    tail = b""
    with open(path, "rb") as f:
        for b in stream_blocks(f, block_bytes):
            text = tail + b if tail else b
            r = ctx.fa_parse(text, 0)
            records += records_of(ctx, r)
            tail = text[r.consumed:]
    records += records_of(ctx, ctx.fa_parse(tail, abi.FA_FINISHED))
    return records
