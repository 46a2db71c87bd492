"""Recall and validation of a signature image: the builder's last step.

build_signature_kmers.cc --recall-output DIR runs every training protein back
through the image it has just written and writes each protein's call and every
annotation that changed (:900-978, :1386-1433); --validation-folder DIR does
the same for held-out genomes (DIR/seq/* FASTA, DIR/anno/* id<TAB>function)
and prints correct / incorrect / missing per file (:984-1026, :1435-1491).
Here the pass, the comparison with the labels and the tallies run on the
device (abi.Recall, csrc/kgx_recall.hip); the host keeps the
names and writes the text.

A sequence's label is its function's index in the function index, LABEL_OTHER
when its id has a function that is not in the index, LABEL_NONE when it has
none.  The device compares indices; the files compare strings, as the
reference does.  The two differ only where a definition's function string is
itself what a call without an index prints -- a "larger ?? smaller" composite
of two indexed names: the totals then count the sequence as changed (its label
is OTHER, no call matches it) while New/ skips the row whose two strings are
equal.  The files follow strings and the totals follow indices.

Beyond the reference, the recall directory also receives functions.tsv
(index, function, labelled, correct, called: recall is correct / labelled,
precision correct / called) and confusions.tsv (label, called, count: the
mislabelled calls by pair of function indices).

    python -m close_kmers_amd.recall --data DATA_DIR --definitions defs.tsv [more.tsv ...] \\
        [--fasta genome1.fa ... --recall-output DIR] [--validation-folder DIR [--validation-verbose]] \\
        [--recall-min-hits 5] [--recall-max-gap 200]

recalls against an existing data directory; python -m close_kmers_amd.signatures
takes the same options and recalls the image it has just built.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

from . import signatures

LABEL_OTHER, LABEL_NONE = -1, -2


def labels(id_function: dict[bytes, bytes], records, functions: list[bytes]) -> np.ndarray:
    """The three-valued label of every record of `records` (a list, per FASTA
    file, of (id, sequence) lists), in order: the index of the id's function
    in `functions`, LABEL_OTHER for a function outside it, LABEL_NONE for an
    id without a function."""
    index = {f: i for i, f in enumerate(functions)}
    out = []
    for recs in records:
        for rid, _ in recs:
            func = id_function.get(rid, b"")
            out.append(index.get(func, LABEL_OTHER) if func else LABEL_NONE)
    return np.asarray(out, np.int32)


def pack(records):
    """residues (uint8) and offsets (uint64) of the records, in order."""
    seqs = [seq for recs in records for _, seq in recs]
    off = np.zeros(len(seqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    return np.frombuffer(b"".join(seqs), np.uint8), off


def format_float(x) -> bytes:
    """A float as the reference's ostream prints it (precision 6, %g): what
    kgx_format_g6 gives."""
    return b"%g" % float(np.float32(x))


def call_function(best_row, functions: list[bytes]) -> bytes:
    """find_best_call's function string from a kgx_best_call (the kinds of kgx.h)."""
    kind = int(best_row["kind"])
    if kind == 1:
        return functions[int(best_row["fi0"])]
    if kind == 2:
        f1, f2 = functions[int(best_row["fi0"])], functions[int(best_row["fi1"])]
        if f2 > f1:
            f1, f2 = f2, f1
        return f1 + b" ?? " + f2
    return b""


def write_recall(out_dir: str, fasta_paths, records, id_function: dict[bytes, bytes], functions: list[bytes],
                 best: np.ndarray, changed) -> None:
    """recall_fasta's two files per FASTA file: out_dir/Calls/<leaf> holds
    id, function, score, weighted_score of every record; out_dir/New/<leaf>
    holds id, old, new of the changed records (`changed`: ascending indices
    into the records of all files, as abi.Recall.changed gives them).  `old` is
    the definitions' string, not the kept index, and a row whose two strings
    are equal is skipped: that happens only for a definition that is itself a
    "larger ?? smaller" composite.  The files follow strings, the totals
    (abi.Recall.stats) follow indices."""
    calls_dir, new_dir = os.path.join(out_dir, "Calls"), os.path.join(out_dir, "New")
    os.makedirs(calls_dir, exist_ok=True)
    os.makedirs(new_dir, exist_ok=True)
    is_changed = np.zeros(len(best), bool)
    is_changed[np.asarray(changed, np.int64)] = True
    at = 0
    for path, recs in zip(fasta_paths, records):
        leaf = os.path.basename(path)
        calls, new = [], []
        for rid, _ in recs:
            b = best[at]
            func = call_function(b, functions)
            calls.append(b"%s\t%s\t%s\t%s\n" % (rid, func, format_float(b["score"]), format_float(b["weighted_score"])))
            if is_changed[at]:
                old = id_function.get(rid, b"")
                if old != func:
                    new.append(b"%s\t%s\t%s\n" % (rid, old, func))
            at += 1
        with open(os.path.join(calls_dir, leaf), "wb") as f:
            f.write(b"".join(calls))
        with open(os.path.join(new_dir, leaf), "wb") as f:
            f.write(b"".join(new))
    if at != len(best):
        raise ValueError(f"{len(best)} best calls for {at} records")


def write_report(out_dir: str, functions: list[bytes], per_function: np.ndarray, confusions: np.ndarray) -> None:
    """functions.tsv and confusions.tsv (see the module's docstring)."""
    with open(os.path.join(out_dir, "functions.tsv"), "wb") as f:
        for i, (name, r) in enumerate(zip(functions, per_function)):
            f.write(b"%d\t%s\t%d\t%d\t%d\n" % (i, name, int(r["labelled"]), int(r["correct"]), int(r["called"])))
    with open(os.path.join(out_dir, "confusions.tsv"), "wb") as f:
        for r in confusions:
            f.write(b"%d\t%d\t%d\n" % (int(r["label"]), int(r["called"]), int(r["count"])))


def recall(ctx, out_dir: str, fasta_paths, records, id_function, functions, params=None,
           piece_residues: int = 0) -> dict:
    """Runs the records through ctx's image and writes out_dir; returns the
    totals (cell as nested lists)."""
    from . import abi
    res, off = pack(records)
    lab = labels(id_function, records, functions)
    os.makedirs(out_dir, exist_ok=True)
    with abi.Recall(ctx, res, off, lab, len(functions), params, piece_residues) as r:
        stats = r.stats()
        write_recall(out_dir, fasta_paths, records, id_function, functions, r.best(), r.changed())
        write_report(out_dir, functions, r.functions(), r.confusions())
    stats["cell"] = stats["cell"].tolist()
    return stats


def read_fasta_all(path) -> list[tuple[bytes, bytes]]:
    """signatures.read_fasta without dropping the records whose id is empty."""
    recs: list[tuple[bytes, list[bytes]]] = []
    with open(path, "rb") as f:
        for line in f.read().split(b"\n"):
            line = line.rstrip(b"\r")
            if line.startswith(b">"):
                word = line[1:].split()
                recs.append((word[0] if word else b"", []))
            elif recs:
                recs[-1][1].append(b"".join(line.split()))
    return [(rid, b"".join(parts)) for rid, parts in recs]


def validation_line(name: str, count: int, cell, missing: int) -> str:
    """validate_fasta's line from a file's cells: correct = kept / match +
    none / none (both strings empty in the second), incorrect = every other
    cell; count includes the records without an id, which never reach the
    device."""
    cell = np.asarray(cell, np.int64).reshape(3, 4)
    correct = int(cell[0, 0] + cell[2, 3])
    return f"{name}: count={count} correct={correct} incorrect={int(cell.sum()) - correct} missing={missing}"


def _regular_files(directory: str) -> list[str]:
    paths = (os.path.join(directory, name) for name in os.listdir(directory))
    return sorted(p for p in paths if os.path.isfile(p))


def validate(ctx, folder: str, functions: list[bytes], params=None, verbose: bool = False, out=None) -> list[str]:
    """validate_fasta over folder/seq/* (in name order) against the
    annotations of folder/anno/*, loaded like definitions; prints and returns
    one line per seq file.  verbose: also "incorrect, id, correct function,
    new function" per miscalled record."""
    from . import abi
    out = out or sys.stdout
    correct = signatures.read_definitions(_regular_files(os.path.join(folder, "anno")))
    lines = []
    for path in _regular_files(os.path.join(folder, "seq")):
        every = read_fasta_all(path)
        recs = [[(rid, seq) for rid, seq in every if rid]]
        missing = len(every) - len(recs[0]) if correct.get(b"", b"") else 0
        res, off = pack(recs)
        lab = labels(correct, recs, functions)
        with abi.Recall(ctx, res, off, lab, len(functions), params) as r:
            cell = r.stats()["cell"]
            if verbose:
                best = r.best()
                for i, (rid, _) in enumerate(recs[0]):
                    new, want = call_function(best[i], functions), correct.get(rid, b"")
                    if new != want:
                        print("incorrect\t%s\t%s\t%s" % (rid.decode(errors="replace"), want.decode(errors="replace"),
                                                         new.decode(errors="replace")), file=out)
        lines.append(validation_line(path, len(every), cell, missing))
        print(lines[-1], file=out)
    return lines


def read_function_index(data_dir: str) -> list[bytes]:
    """function.index ("%d\\t%s\\n", dense and in order) as the list of names."""
    names = []
    with open(os.path.join(data_dir, "function.index"), "rb") as f:
        for line in f.read().split(b"\n"):
            if not line:
                continue
            num, _, name = line.partition(b"\t")
            if int(num) != len(names):
                raise ValueError("function.index must be dense and in order")
            names.append(name)
    return names


def add_arguments(ap: argparse.ArgumentParser) -> None:
    """The reference's recall options and defaults (build_signature_kmers.cc:1100-1118)."""
    ap.add_argument("--recall-output", help="directory for Calls/, New/, functions.tsv and confusions.tsv")
    ap.add_argument("--validation-folder", help="directory with seq/ (FASTA) and anno/ (id<TAB>function)")
    ap.add_argument("--validation-verbose", action="store_true", help="print every incorrect validation call")
    ap.add_argument("--recall-min-hits", type=int, default=5)
    ap.add_argument("--recall-max-gap", type=int, default=200)


def run(ctx, a, fasta_paths, records, id_function, functions) -> dict:
    """What the options of add_arguments ask for, on ctx's image."""
    params = {"min_hits": a.recall_min_hits, "max_gap": a.recall_max_gap}
    out = {}
    if a.recall_output:
        out["recall"] = recall(ctx, a.recall_output, fasta_paths, records, id_function, functions, params)
    if a.validation_folder:
        out["validation"] = validate(ctx, a.validation_folder, functions, params, a.validation_verbose)
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m close_kmers_amd.recall",
                                 description="Recall labelled proteins against a kmer data directory.")
    ap.add_argument("--data", required=True, help="kmer data directory (kmer.table.mem_map, function.index)")
    ap.add_argument("--definitions", nargs="+", default=[], help="id<TAB>function files, later ones override")
    ap.add_argument("--fasta", nargs="+", default=[], help="protein FASTA files")
    ap.add_argument("--device", type=int, default=0)
    add_arguments(ap)
    a = ap.parse_args(argv)
    if not a.recall_output and not a.validation_folder:
        ap.error("one of --recall-output and --validation-folder is needed")
    from . import abi
    functions = read_function_index(a.data)
    id_function = signatures.read_definitions(a.definitions)
    records = [signatures.read_fasta(p) for p in a.fasta]
    with abi.Image.open(a.data, a.device) as img, abi.Context(img) as ctx:
        out = run(ctx, a, a.fasta, records, id_function, functions)
    if "recall" in out:
        print(json.dumps(out["recall"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
