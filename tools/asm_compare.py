#!/usr/bin/env python3
"""Compare two builds' device assembly kernel by kernel.

    hipcc <the flags of close_kmers_amd/build.py> --cuda-device-only -S \\
          -Rpass-analysis=kernel-resource-usage csrc/X.hip -o X.s 2> X.remarks     (in both trees)
    tools/asm_compare.py OLD/X.s NEW/X.s --remarks OLD/X.remarks NEW/X.remarks [--json out.json]

For every kernel (a symbol with an .amdhsa_kernel descriptor) the instruction
stream and the descriptor are compared after dropping what is not code:
comments, blank lines, .loc/.file/.cfi lines and the numbering of local
labels.  Symbol order does not matter: kernels are matched by name.  With
--remarks the compiler's resource remarks (registers, scratch, LDS,
occupancy) are compared the same way.  Exit status 1 when anything differs.
Text only: it needs no GPU and runs nothing.
"""
import argparse
import json
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_begin|func_end|tmp|JTI)\d+(_\d+)?")


def _clean(line):
    line = line.split(";", 1)[0].split("//", 1)[0].strip()
    if not line or re.match(r"\.(loc|file|cfi_\w+|ident|section|text|globl|protected|weak|type|size)\b", line):
        return None
    return line


def kernels(path):
    """name -> {"code": [lines], "descriptor": [lines]}, labels numbered per kernel in order of appearance"""
    text = open(path).read().splitlines()
    names = [m.group(1) for ln in text for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)] if m]
    out = {n: {"code": [], "descriptor": []} for n in names}
    cur, part = None, None
    for raw in text:
        m = re.match(r"(\S+):\s*(;.*)?$", raw)
        if m and m.group(1) in out and part is None:
            cur, part = m.group(1), "code"
            continue
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", raw)
        if m:
            cur, part = m.group(1), "descriptor"
            continue
        if part == "code" and re.match(r"\.Lfunc_end\d+:", raw.strip()):
            part = None
            continue
        if part == "descriptor" and raw.strip() == ".end_amdhsa_kernel":
            part = None
            continue
        if part:
            ln = _clean(raw)
            if ln:
                out[cur][part].append(ln)
    for k in out.values():
        seen = {}
        k["code"] = [LOCAL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), ln) for ln in k["code"]]
    return out


def remarks(path):
    """name -> {resource: value} from -Rpass-analysis=kernel-resource-usage"""
    out, name = {}, None
    for ln in open(path):
        m = re.search(r"remark: (?:\S+: )?Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r"remark:\s+(?:\S+:\d+:\d+:\s+)?([A-Za-z][^:]*): (\d+)", ln)
        if m and name:
            out[name][m.group(1).strip()] = int(m.group(2))
    return out


def instructions(code):
    return sum(1 for ln in code if not ln.endswith(":") and not ln.startswith("."))


def compare(old_s, new_s, old_r=None, new_r=None):
    a, b = kernels(old_s), kernels(new_s)
    ra, rb = (remarks(old_r), remarks(new_r)) if old_r else ({}, {})
    res = {"old_kernels": len(a), "new_kernels": len(b), "compared": 0, "identical": 0,
           "only_old": sorted(set(a) - set(b)), "only_new": sorted(set(b) - set(a)), "differing": []}
    for name in sorted(set(a) & set(b)):
        res["compared"] += 1
        what = [p for p in ("code", "descriptor") if a[name][p] != b[name][p]]
        if old_r and ra.get(name) != rb.get(name):
            what.append("resources")
        if not what:
            res["identical"] += 1
            continue
        res["differing"].append({"kernel": name, "differs_in": what,
                                 "old_instructions": instructions(a[name]["code"]),
                                 "new_instructions": instructions(b[name]["code"]),
                                 "old_resources": ra.get(name), "new_resources": rb.get(name)})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_s")
    ap.add_argument("new_s")
    ap.add_argument("--remarks", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--json")
    args = ap.parse_args()
    res = compare(args.old_s, args.new_s, *(args.remarks or (None, None)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "differing"}))
    for d in res["differing"]:
        print("DIFFERS", d["kernel"], d["differs_in"], d["old_instructions"], "->", d["new_instructions"])
    return 1 if res["differing"] or res["only_old"] or res["only_new"] else 0


if __name__ == "__main__":
    sys.exit(main())
