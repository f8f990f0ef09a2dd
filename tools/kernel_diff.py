#!/usr/bin/env python3
"""Per-kernel comparison of the device assembly of two revisions of the kernel files -- the check a refactor of a .hip file
or of a header it includes is held to (profiles/search_split.json, profiles/front_end_shared.json).

    python tools/kernel_diff.py --parent HEAD [--out FILE.json] [FILE.hip ...]

The parent revision is checked out with `git worktree` into a temporary directory; both sides of every file are compiled
with the Makefile's own flags (its per-file additions included, such as the search's -fno-slp-vectorize) plus
-S --cuda-device-only.  Per kernel the body runs from its label to its .Lfunc_end; comment, directive and local-label
lines are dropped, and so are references to local labels (their numbers count the functions of the file, so they shift
when a neighbour changes).  Reported per kernel: LDS (group segment) and scratch (private segment) bytes, next free VGPR
and SGPR, the number of instruction lines, and "identical" or the first differing line.  Text is compared, nothing is run:
no GPU is needed, and no instruction is looked for.

Without FILE arguments every .hip file that includes mh_device.h -- directly or through a header -- is compared."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("monohair_amd", "csrc")
RESOURCES = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr", "next_free_sgpr", "accum_offset")


def make_flags(csrc, obj):
    """hipcc and the flags `make` would compile `obj` with, read from make's own database (-n: nothing is built)."""
    db = subprocess.run(["make", "-C", csrc, "-npB", obj], capture_output=True, text=True).stdout
    hipcc = re.search(r"^HIPCC\s*\??=\s*(\S+)", db, re.M).group(1)
    line = next(l for l in db.splitlines() if l.startswith(hipcc) and " -c " in l and l.rstrip().endswith("-o " + obj))
    return [hipcc] + [w for w in line.split()[1:] if w not in ("-c", "-o", obj) and not w.endswith(".hip")]


def includes_device_header(csrc, name, seen=None):
    seen = set() if seen is None else seen
    if name in seen or not os.path.exists(os.path.join(csrc, name)):
        return False
    seen.add(name)
    text = open(os.path.join(csrc, name)).read()
    incs = re.findall(r'^\s*#\s*include\s+"([^"/]+)"', text, re.M)
    return "mh_device.h" in incs or any(includes_device_header(csrc, i, seen) for i in incs)


def assemble(csrc, hip, out_dir):
    obj = hip[:-4] + ".o"
    asm = os.path.join(out_dir, hip[:-4] + ".s")
    subprocess.check_call(make_flags(csrc, obj) + ["-S", "--cuda-device-only", hip, "-o", asm], cwd=csrc)
    return open(asm).read()


def demangle(names):
    if not names:
        return {}
    tool = shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin:/opt/rocm/lib/llvm/bin") or shutil.which("c++filt")
    plain = names
    if tool:
        out = subprocess.run([tool] + names, capture_output=True, text=True)
        plain = out.stdout.split("\n")[:len(names)] if out.returncode == 0 else names
    # the argument list of a kernel says nothing its name and template arguments do not
    return {n: re.sub(r"\(.*\)$", "", p) for n, p in zip(names, plain)}


def kernels_of(asm):
    """{kernel symbol: (instruction lines, resources)} of one device assembly file."""
    lines = asm.split("\n")
    labels = {l.split(";")[0].strip(): i for i, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ".")}
    res = {}
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", asm, re.S):
        res[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+)\s+(\d+)", m.group(2)) if k in RESOURCES}
    out = {}
    for sym in res:
        start = labels[sym + ":"]
        body = []
        for l in lines[start + 1:]:
            s = l.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or s.startswith(".") or s.endswith(":"):   # comment, directive, (local) label
                continue
            body.append(re.sub(r"\.L\w+", ".L", " ".join(s.split())))
        out[sym] = (body, res[sym])
    return out


def compare(parent_asm, change_asm):
    pk, ck = kernels_of(parent_asm), kernels_of(change_asm)
    names = demangle(sorted(set(pk) | set(ck)))
    report = {}
    for sym in sorted(names, key=lambda s: names[s]):
        if sym not in pk or sym not in ck:
            report[names[sym]] = {"outcome": "only in " + ("change" if sym in ck else "parent")}
            continue
        (pb, pr), (cb, cr) = pk[sym], ck[sym]
        first = next((i for i, (a, b) in enumerate(zip(pb, cb)) if a != b), None)
        if first is None and len(pb) != len(cb):
            first = min(len(pb), len(cb))
        report[names[sym]] = {
            "outcome": "identical" if first is None else "differs",
            "instruction_lines": [len(pb), len(cb)],
            "first_difference": None if first is None else {
                "line": first, "parent": pb[first] if first < len(pb) else None,
                "change": cb[first] if first < len(cb) else None},
            "resources_equal": pr == cr,
            "resources_not_worse": all(cr[k] <= pr[k] for k in RESOURCES[:3]),   # LDS, scratch, VGPRs
            "parent": pr, "change": cr}
    return report


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--parent", default="HEAD", help="revision to compare the working tree against")
    ap.add_argument("--out", help="write the report as JSON here (a summary is always printed)")
    ap.add_argument("files", nargs="*", help=".hip files of monohair_amd/csrc (default: all that include mh_device.h)")
    args = ap.parse_args()
    csrc = os.path.join(ROOT, CSRC)
    files = [os.path.basename(f) for f in args.files] or sorted(
        f for f in os.listdir(csrc) if f.endswith(".hip") and includes_device_header(csrc, f))
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", args.parent], text=True).strip()
    report = {"parent_commit": commit, "how": "both sides compiled with the Makefile's flags plus -S --cuda-device-only; per "
              "kernel the body from its label to its end, comment, directive and local-label lines dropped, local label "
              "references made anonymous", "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        tree = os.path.join(tmp, "parent")
        subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", "--force", tree, commit],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        try:
            for f in files:
                if not os.path.exists(os.path.join(tree, CSRC, f)):
                    report["files"][f] = {"outcome": "not in the parent"}
                    continue
                os.makedirs(os.path.join(tmp, "p"), exist_ok=True)
                os.makedirs(os.path.join(tmp, "c"), exist_ok=True)
                report["files"][f] = compare(assemble(os.path.join(tree, CSRC), f, os.path.join(tmp, "p")),
                                             assemble(csrc, f, os.path.join(tmp, "c")))
        finally:
            subprocess.call(["git", "-C", ROOT, "worktree", "remove", "--force", tree],
                            stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    bad = 0
    for f, ks in report["files"].items():
        if "outcome" in ks:
            print("%s: %s" % (f, ks["outcome"]))
            continue
        same = sum(k["outcome"] == "identical" for k in ks.values())
        print("%s: %d kernels, %d identical" % (f, len(ks), same))
        for name, k in ks.items():
            if k["outcome"] == "identical":
                continue
            worse = "instruction_lines" in k and not k["resources_not_worse"]
            bad += worse
            if "instruction_lines" not in k:
                print("   %-60s %s" % (name, k["outcome"]))
                continue
            p, c = k["parent"], k["change"]
            print("   %-60s lines %d -> %d  vgpr %d -> %d  sgpr %d -> %d  lds %d -> %d  scratch %d -> %d%s" % (
                name, k["instruction_lines"][0], k["instruction_lines"][1], p["next_free_vgpr"], c["next_free_vgpr"],
                p["next_free_sgpr"], c["next_free_sgpr"], p["group_segment_fixed_size"], c["group_segment_fixed_size"],
                p["private_segment_fixed_size"], c["private_segment_fixed_size"], "   RESOURCES WORSE" if worse else ""))
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(report, fh, indent=1, sort_keys=True)
            fh.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
