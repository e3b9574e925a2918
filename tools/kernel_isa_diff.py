#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel (CPU only).

    python tools/kernel_isa_diff.py --old OLD/*.s --new NEW/*.s [--must-match REGEX]

OLD and NEW are the `.s` files of `make -C gpu-ray-tracing_amd asm` from two trees.  Kernels are
paired by mangled name, whichever file they live in, so a kernel that moved to another
translation unit is compared with itself.  Of each kernel the whole instruction stream is
compared after stripping comments, directives and the function ordinal of basic-block labels
(`.LBB12_3` -> `.LBB_3`); the registers, scratch, LDS and occupancy come from the compiler's
"Kernel info" notes after it.  Prints one line per kernel and exits 1 if a kernel whose name
matches --must-match differs or is missing on either side.
"""
import argparse
import difflib
import re
import sys

NOTES = (("vgpr", "NumVgprs"), ("sgpr", "TotalNumSgprs"), ("scratch", "ScratchSize"),
         ("lds", "LDSByteSize"), ("occ", "Occupancy"))


def kernels(paths):
    """{mangled name: (instruction lines, {note: value})} of every .amdhsa_kernel in paths."""
    out = {}
    for path in paths:
        text = open(path).read()
        for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M):
            body = text.split("\n%s:" % name, 1)[1].split("\n\t.end_amdhsa_kernel", 1)
            lines = []
            for line in body[0].split("\n")[1:]:
                line = re.sub(r"\s+", " ", line.split(";", 1)[0]).strip()
                if line and not (line.startswith(".") and not line.endswith(":")):
                    lines.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", line))
            info = body[1].split("; Kernel info:", 1)[1]
            notes = {k: int(re.search(r"; %s: (\d+)" % n, info).group(1)) for k, n in NOTES}
            out[name] = (lines, notes)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--must-match", default=None, metavar="REGEX")
    a = ap.parse_args()
    old, new = kernels(a.old), kernels(a.new)
    must = re.compile(a.must_match) if a.must_match else None
    failed = 0
    for name in sorted(set(old) | set(new)):
        sides = [("%(vgpr)d v %(sgpr)d s scratch %(scratch)d lds %(lds)d occ %(occ)d" % k[name][1])
                 if name in k else "missing" for k in (old, new)]
        if name in old and name in new:
            n = sum(1 for d in difflib.ndiff(old[name][0], new[name][0]) if d[0] in "+-")
            verdict = "same" if n == 0 else "differs (%d lines)" % n
        else:
            verdict = "missing"
        pinned = bool(must and must.search(name))
        failed += pinned and verdict != "same"
        print("%-20s %s%s\n    old: %s\n    new: %s" % (verdict, name, "  [must match]" if pinned else "",
                                                       sides[0], sides[1]))
    print("%d kernels, %d pinned by --must-match failed" % (len(set(old) | set(new)), failed))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
