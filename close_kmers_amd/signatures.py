"""From function definitions and FASTA files to a kmer data directory.

The front end of build_signature_kmers.cc over the device selection
(abi.Signatures, csrc/kgx_sig.hip):

  * definitions: id -> function from the first two tab-separated columns of
    each file, later files overriding earlier ones (load_id_assignments,
    build_signature_kmers.cc:270-295; a line without a tab is skipped);
  * FASTA: one genome per file; a function occurs in a genome when one of the
    file's ids has it (load_fasta_file :308-414);
  * process_kept_functions (:432-488): a function is kept when it occurs in
    at least min_reps genomes (default 5) or is in the caller's list; kept
    functions are numbered in sorted (byte) order;
  * every sequence whose id has a kept function is labelled with its number,
    every other with -1, and the whole corpus goes through one selection;
  * the directory receives function.index ("%d\\t%s\\n"), an empty otu.index,
    the reference's placeholder `genomes` file and kmer.table.mem_map, the
    files KmerImage / kgx_image_open and the handlers read.

--recall-output DIR and --validation-folder DIR run the builder's last step,
the recall of the training proteins and the validation of held-out genomes, on
the image just built, before it is closed (close_kmers_amd/recall.py,
DESIGN.md §8.9).

Left out, as in DESIGN.md §8.8: good roles (a function kept because one of its
roles is listed), stripping of function comments ("# ..." / "! ..." tails),
and functions or genome names taken from FASTA definition lines (the
"[genome]" regex); a function here is exactly the definitions' second column.

    python -m close_kmers_amd.signatures --definitions defs.tsv [more.tsv ...] \\
        --fasta genome1.fa genome2.fa ... [--min-reps 5] [--keep-function NAME ...] --out DIR \\
        [--max-pass-tuples N] [--recall-output DIR] [--validation-folder DIR [--validation-verbose]] \\
        [--recall-min-hits 5] [--recall-max-gap 200]

A corpus whose tuples do not fit the device at once is selected in passes over
key ranges with the same result; --max-pass-tuples bounds a
pass by hand, and the printed statistics say how many passes ran (n_passes).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import synth


def read_definitions(paths) -> dict[bytes, bytes]:
    """id -> function over the files in order; later lines and files win."""
    out: dict[bytes, bytes] = {}
    for path in paths:
        with open(path, "rb") as f:
            for line in f.read().split(b"\n"):
                cols = line.split(b"\t")
                if len(cols) < 2:
                    continue
                out[cols[0]] = cols[1]
    return out


def read_fasta(path) -> list[tuple[bytes, bytes]]:
    """(id, sequence) records: the id is the definition line's first word."""
    recs: list[tuple[bytes, list[bytes]]] = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            line = line.rstrip(b"\r")
            if line.startswith(b">"):
                word = line[1:].split()
                recs.append((word[0] if word else b"", []))
            elif recs:
                recs[-1][1].append(b"".join(line.split()))
    return [(rid, b"".join(parts)) for rid, parts in recs if rid]


def kept_functions(id_function: dict[bytes, bytes], genomes: list[list[bytes]], min_reps: int = 5,
                   keep=()) -> list[bytes]:
    """process_kept_functions: genomes[g] lists the ids of genome g; returns
    the kept functions in index order."""
    seen: dict[bytes, set[int]] = {}
    for g, ids in enumerate(genomes):
        for rid in ids:
            func = id_function.get(rid, b"")
            if func:
                seen.setdefault(func, set()).add(g)
    wanted = {k.encode() if isinstance(k, str) else bytes(k) for k in keep}
    return sorted(f for f, gs in seen.items() if len(gs) >= min_reps or f in wanted)


def function_index_bytes(functions: list[bytes]) -> bytes:
    """write_function_index, build_signature_kmers.cc:519-529."""
    return b"".join(b"%d\t%s\n" % (i, f) for i, f in enumerate(functions))


def table_size(n_kept: int) -> int:
    """write_hashtable's size: the first listed prime above 3 * n_kept."""
    return synth.builder_num_sigs(n_kept)


def label(id_function: dict[bytes, bytes], fastas: list[list[tuple[bytes, bytes]]], functions: list[bytes]):
    """The corpus as the selection takes it: residues, offsets, seq_function."""
    index = {f: i for i, f in enumerate(functions)}
    seqs, fn = [], []
    for recs in fastas:
        for rid, seq in recs:
            seqs.append(seq)
            fn.append(index.get(id_function.get(rid, b""), -1))
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    res = np.frombuffer(b"".join(seqs), np.uint8)
    return res, off, np.asarray(fn, np.int32)


def write_indexes(out_dir: str, functions: list[bytes]) -> None:
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "function.index"), "wb") as f:
        f.write(function_index_bytes(functions))
    open(os.path.join(out_dir, "otu.index"), "wb").close()
    with open(os.path.join(out_dir, "genomes"), "wb") as f:
        f.write(b"empty genomes\n")  # build_signature_kmers.cc:1313-1321


def build_data_dir(definitions, fastas, out_dir: str, min_reps: int = 5, keep=(), device: int = 0,
                   num_sigs: int = 0, max_pass_tuples: int = 0, recall_output: str | None = None,
                   validation_folder: str | None = None, validation_verbose: bool = False,
                   recall_min_hits: int = 5, recall_max_gap: int = 200) -> dict:
    """Runs the whole builder on `device`; returns the selection's statistics
    with n_functions, n_stored and n_passes added.  max_pass_tuples: the most
    tuples one pass of the selection holds (0: what the device holds).
    recall_output / validation_folder: the image, while it is still held, also
    recalls the corpus into that directory / validates that folder's genomes
    (recall.recall, recall.validate); the totals are returned under "recall" /
    "validation"."""
    from . import abi, recall
    id_function = read_definitions(definitions)
    records = [read_fasta(p) for p in fastas]
    functions = kept_functions(id_function, [[rid for rid, _ in recs] for recs in records], min_reps, keep)
    res, off, fn = label(id_function, records, functions)
    write_indexes(out_dir, functions)
    with abi.Signatures(res, off, fn, len(functions), device, max_pass_tuples=max_pass_tuples) as sig:
        stats = sig.stats()
        n_passes = len(sig.passes())
        img, stored = sig.image(num_sigs)
        with img:
            img.save(out_dir)
            if recall_output or validation_folder:
                params = {"min_hits": recall_min_hits, "max_gap": recall_max_gap}
                with abi.Context(img) as ctx:
                    if recall_output:
                        stats["recall"] = recall.recall(ctx, recall_output, fastas, records, id_function, functions,
                                                        params)
                    if validation_folder:
                        stats["validation"] = recall.validate(ctx, validation_folder, functions, params,
                                                              validation_verbose)
    stats.update(n_functions=len(functions), n_stored=stored, n_passes=n_passes)
    return stats


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.signatures", description=__doc__.split("\n\n")[0])
    ap.add_argument("--definitions", nargs="+", required=True, help="id<TAB>function files, later ones override")
    ap.add_argument("--fasta", nargs="+", required=True, help="protein FASTA files, one genome each")
    ap.add_argument("--min-reps", type=int, default=5, help="genomes a function must occur in (default 5)")
    ap.add_argument("--keep-function", action="append", default=[], help="a function kept regardless (repeatable)")
    ap.add_argument("--out", required=True, help="kmer data directory to write")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--num-sigs", type=int, default=0, help="table size (default: the builder's prime rule)")
    ap.add_argument("--max-pass-tuples", type=int, default=0,
                    help="most tuples held on the device at once (default: what it holds, at most 2^31-1)")
    from . import recall
    recall.add_arguments(ap)
    a = ap.parse_args(argv)
    stats = build_data_dir(a.definitions, a.fasta, a.out, a.min_reps, a.keep_function, a.device, a.num_sigs,
                           a.max_pass_tuples, a.recall_output, a.validation_folder, a.validation_verbose,
                           a.recall_min_hits, a.recall_max_gap)
    print(json.dumps(stats))
    return 0


if __name__ == "__main__":
    sys.exit(main())
