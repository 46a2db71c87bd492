"""Proteins grouped by their signature k-mer sets: the reference's unique_prots.

unique_prots.cc (:61-109) reads a protein FASTA, collects per protein the set
of signature k-mers the image hits in it (hit.which_kmer through hit_cb, so
before every scoring rule) and prints the proteins grouped by identical set,
in the order of std::map<std::set<unsigned long long>, std::vector<std::string>>:
per group every id followed by a tab, then a newline.  Here the sets, the
grouping and the order are made on the device (abi.Unique, csrc/kgx_uniq.hip,
DESIGN.md §8.10); the host reads the FASTA and writes the text.

    python -m close_kmers_amd.unique_prots DATA_DIR FASTA [FASTA ...] [--device N] [--output FILE] \\
        [--piece-residues N] [--parse-device]

Several FASTA files are read as one input, in order.  Ids are the definition
lines' first words; a record with an empty id is kept, as the reference's
parser calls back for it.  With --parse-device (off by default) the files are
framed by the device parser (fasta_device.read_records), so
the records are the reference's FastaParser's where the host reader differs:
"> x" has an empty id, a byte the parser reports is dropped.
"""
from __future__ import annotations

import argparse
import sys

from . import recall


def format_groups(ids, group_offsets, members) -> bytes:
    """The reference's text of the groups (a CSR of indices into ids)."""
    out = []
    for g in range(len(group_offsets) - 1):
        for i in members[int(group_offsets[g]):int(group_offsets[g + 1])]:
            out.append(ids[int(i)])
            out.append(b"\t")
        out.append(b"\n")
    return b"".join(out)


def unique(ctx, records, piece_residues: int = 0):
    """(text, stats) of the records (a list, per FASTA file, of (id, sequence)
    lists) over ctx's image."""
    from . import abi
    res, off = recall.pack(records)
    ids = [rid for recs in records for rid, _ in recs]
    with abi.Unique(ctx, res, off, piece_residues) as u:
        group_offsets, members = u.groups()
        return format_groups(ids, group_offsets, members), u.stats()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.unique_prots",
                                 description="Group proteins by the set of signature k-mers they hit.")
    ap.add_argument("data", metavar="DATA_DIR", help="kmer data directory (kmer.table.mem_map)")
    ap.add_argument("fasta", metavar="FASTA", nargs="+", help="protein FASTA files, read as one input")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--output", help="file for the text (default: stdout)")
    ap.add_argument("--piece-residues", type=int, default=0, help="residues per device piece (0: the library's default)")
    ap.add_argument("--parse-device", action="store_true",
                    help="frame the FASTA files on the device, as the reference's parser frames them (default: off)")
    a = ap.parse_args(argv)
    from . import abi
    if not a.parse_device:
        records = [recall.read_fasta_all(p) for p in a.fasta]
    with abi.Image.open(a.data, a.device) as img, abi.Context(img) as ctx:
        if a.parse_device:
            from . import fasta_device
            records = [fasta_device.read_records(ctx, p) for p in a.fasta]
        text, _ = unique(ctx, records, a.piece_residues)
    if a.output:
        with open(a.output, "wb") as f:
            f.write(text)
    else:
        sys.stdout.buffer.write(text)
        sys.stdout.buffer.flush()
    return 0


if __name__ == "__main__":
    sys.exit(main())
