#!/usr/bin/env python3
"""Which vmcnt waits stand before the table writes and the first butterfly of
the wave-staged pass kernels (rs16_pass.hpp WaveStaged)?

    scripts/staging_waits.py rs16_pass_enc.s

The .s is the device assembly of rs16_pass_enc.hip (the Makefile's flags plus
`--cuda-device-only -S`).  The speed of those kernels rests on the compiler's
wait insertion: the tables must be written with every row load still in
flight (vmcnt >= 2 x 16 rows) and the first butterfly must wait for its own
rows only (vmcnt 28: rows 0, 1; ENC_LAST 14: rows 0, 8).  A control-flow shape
that leaves a path without row loads turns both into vmcnt(0) without any
other sign.  Per kernel, on the straight-line path from the full-item row
requests on: the last vmcnt wait before the first ds_write_b128, the last
one before the first v_perm_b32, and whether an s_barrier precedes that
v_perm.  Exit status 1 if any differs from the expected values.
"""
import re
import sys

KERNEL = re.compile(r"^_ZN4rs1611pass_kernelILi([234])ELi([78])ELi(\d)EEEvNS_8PassArgsE:")
NAMES = {"2": "ENC_FIRST", "3": "ENC_MID", "4": "ENC_LAST"}
VM = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")


def main():
    lines = open(sys.argv[1]).read().splitlines()
    bad = 0
    i = 0
    while i < len(lines):
        m = KERNEL.match(lines[i])
        if not m:
            i += 1
            continue
        name = "pass_kernel<%s,%s,%s>" % (NAMES[m.group(1)], m.group(2), m.group(3))
        # the last "full-item rows requested" marker before the first table write
        j = i
        marker = None
        while not lines[j].startswith(".Lfunc_end"):
            if "full-item rows requested" in lines[j]:
                marker = j
            if marker is not None and "ds_write_b128" in lines[j]:
                break
            j += 1
        wait_tab = wait_bfly = None
        last = None
        barrier = False
        k = marker
        while not lines[k].startswith(".Lfunc_end"):
            t = lines[k].strip()
            w = VM.search(t)
            if w:
                last = int(w.group(1))
            if t.startswith("s_barrier"):
                barrier = True
            if t.startswith("ds_write_b128") and wait_tab is None:
                wait_tab = last
            if t.startswith("v_perm_b32"):
                wait_bfly = last
                break
            k += 1
        want_bfly = 14 if m.group(1) == "4" else 28
        ok = wait_tab is not None and wait_tab >= 32 and wait_bfly == want_bfly and not barrier
        bad += not ok
        print("%-28s tables vmcnt(%s)  first butterfly vmcnt(%s)  barrier before it: %s  %s"
              % (name, wait_tab, wait_bfly, "yes" if barrier else "no", "ok" if ok else "UNEXPECTED"))
        i = k
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
