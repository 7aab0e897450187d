#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?

    scripts/isa_compare.py DIR_A DIR_B

DIR_A and DIR_B hold the device assembly of the two builds, one .s per .hip
file, made with the Makefile's flags plus `--cuda-device-only -S` (and the
per-file FILEFLAGS).  Kernels are matched by symbol over all files of a
directory, so a kernel may move between translation units.  For every kernel
three texts are hashed and compared:

    code  the lines between its label and its .Lfunc_end label
    desc  its .amdhsa_kernel descriptor block
    meta  its entry of the amdgpu_metadata note (kernarg and LDS size,
          register counts, scratch)

Only the function index of local labels is normalised (.LBB<n>_ -> .LBB_) and
comments are stripped.  The script hashes text; it inspects no instruction.
Prints the counts and every differing symbol -- for a kernel whose desc
differs, also the descriptor lines that differ, "- " the first build's and
"+ " the second's; exit status 1 on any difference.
"""
import hashlib
import re
import sys
from pathlib import Path

LBB = re.compile(r"\.LBB\d+_")


def clean(line):
    line = line.split(";", 1)[0].rstrip()
    return LBB.sub(".LBB_", line)


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def kernels_of(path):
    """{symbol: {"code": h, "desc": h, "meta": h, "desc_lines": [...]}} of one .s file."""
    lines = path.read_text().splitlines()
    out = {}
    # descriptor blocks name the kernels; the code of `sym` starts at "sym:"
    label_at = {}
    for i, l in enumerate(lines):
        if l and not l[0].isspace() and l.split(";", 1)[0].rstrip().endswith(":"):
            label_at.setdefault(l.split(":", 1)[0], i)
    i = 0
    while i < len(lines):
        s = lines[i].strip()
        if s.startswith(".amdhsa_kernel "):
            sym = s.split()[1]
            j = i
            while lines[j].strip() != ".end_amdhsa_kernel":
                j += 1
            desc = [clean(l).strip() for l in lines[i:j + 1]]
            start = label_at[sym]
            end = j
            while not re.match(r"\.Lfunc_end\d+:", lines[end]):
                end += 1
            code = [clean(l) for l in lines[start:i] + lines[j + 1:end]]
            out[sym] = {"code": digest([l for l in code if l.strip()]), "desc": digest(desc),
                        "desc_lines": desc}
            i = j
        i += 1
    # metadata note: a YAML list under amdhsa.kernels, one "  - " item per kernel
    try:
        m0 = lines.index("amdhsa.kernels:")
    except ValueError:
        m0 = len(lines)
    item = []

    def flush():
        names = [l.split(":", 1)[1].strip() for l in item if l.startswith("    .name:")]
        if names:
            out[names[0]]["meta"] = digest(item)

    for l in lines[m0 + 1:]:
        if not l.startswith(" "):
            break
        if l.startswith("  - "):
            flush()
            item = []
        item.append(l.rstrip())
    flush()
    return out


def kernels_in(d):
    all_k = {}
    for p in sorted(Path(d).glob("*.s")):
        for sym, h in kernels_of(p).items():
            if sym in all_k:
                sys.exit(f"{d}: kernel {sym} defined twice")
            all_k[sym] = dict(h, file=p.name)
    return all_k


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels_in(sys.argv[1]), kernels_in(sys.argv[2])
    print(f"{sys.argv[1]}: {len(a)} kernels; {sys.argv[2]}: {len(b)} kernels")
    bad = 0
    for sym in sorted(set(a) - set(b)):
        print(f"only in {sys.argv[1]}: {sym} ({a[sym]['file']})")
        bad += 1
    for sym in sorted(set(b) - set(a)):
        print(f"only in {sys.argv[2]}: {sym} ({b[sym]['file']})")
        bad += 1
    same = 0
    for sym in sorted(set(a) & set(b)):
        diff = [k for k in ("code", "desc", "meta") if a[sym].get(k) != b[sym].get(k)]
        if diff:
            print(f"differs ({', '.join(diff)}): {sym} ({a[sym]['file']} / {b[sym]['file']})")
            if "desc" in diff:
                da, db = a[sym]["desc_lines"], b[sym]["desc_lines"]
                for l in da:
                    if l not in db:
                        print(f"    - {l}")
                for l in db:
                    if l not in da:
                        print(f"    + {l}")
            bad += 1
        else:
            same += 1
    print(f"identical: {same}; differing or unmatched: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
