#!/usr/bin/env python3
"""Which vmcnt waits stand before the table writes and the first butterfly of
the wave-staged pass kernels (rs16_pass.hpp WaveStaged)?

    scripts/staging_waits.py rs16_pass_enc.s
    scripts/staging_waits.py rs16_pass_tower.s

The .s is the device assembly of rs16_pass_enc.hip or rs16_pass_tower.hip (the
Makefile's flags plus `--cuda-device-only -S`).  The speed of those kernels rests on the compiler's
wait insertion: the tables must be written with every row load still in
flight (vmcnt >= 2 x 16 rows) and the first butterfly must wait for its own
rows only (vmcnt 28: rows 0, 1; ENC_LAST 14: rows 0, 8).  A control-flow shape
that leaves a path without row loads turns both into vmcnt(0) without any
other sign.  Per kernel, on the straight-line path from the full-item row
requests on: the last vmcnt wait before the first ds_write_b128, the last
one before the first v_perm_b32, and whether an s_barrier precedes that
v_perm.  Exit status 1 if any differs from the expected values.

The late-rows variants (pass_kernel_late, LateRows) request D row pairs ahead
of the table commit (4 D dword loads before the "late rows: prologue
requested" marker; D is read off the assembly) and pair g + D right before
butterfly g of the first layer.  From the marker on, in program order, the
script counts the row loads requested (global_load_dword) and, at every vmcnt
wait, the loads that wait retires.  Expected:

    tables     the last wait before the first ds_write_b128 leaves >= 4 D
               loads in flight (the whole prologue)
    butterfly  at the first v_perm_b32 that follows the retirement of pair g
               (g = 0 .. 7, none skipped), exactly the loads requested after
               pair g are in flight: 4 min(D, 7 - g)
    form       every late request is an SGPR-base load
    no s_barrier, and no vmcnt(0) before the wait for the last pair

The paired-rows flavours (pass_kernel_late_paired) that read paired rows
request a row with one global_load_dwordx2: 2 D requests in the prologue and
exactly 2 min(D, 7 - g) in flight at butterfly g; the rest as above.  (The
flavour of the gathering first pass reads the caller's rows with dword loads
and is checked as the unpaired kernel is.)

The tower flavours (pass_kernel_late_tower, rs16_pass_tower.s) are checked as
the paired flavours of the same programs are: the first pass reads the
caller's rows, the middle and last passes paired rows.  In the last pass the
first v_perm_b32 of butterfly g is the conversion of its rows out of tower
form, which waits for the same pair.
"""
import re
import sys

KERNEL = re.compile(r"^_ZN4rs1611pass_kernelILi([234])ELi([78])ELi(\d)EEEvNS_8PassArgsE:")
LATE = re.compile(r"^_ZN4rs1616pass_kernel_lateILi([234])ELi([78])ELi(\d)EEEvNS_8PassArgsE:")
PAIRED = re.compile(r"^_ZN4rs1623pass_kernel_late_pairedILi([234])ELi([78])ELi(\d)ELb([01])ELb([01])EEEvNS_8PassArgsE:")
TOWER = re.compile(r"^_ZN4rs1622pass_kernel_late_towerILi([234])ELi([78])ELi(\d)EEEvNS_8PassArgsE:")
NAMES = {"2": "ENC_FIRST", "3": "ENC_MID", "4": "ENC_LAST"}
VM = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")
ROW_LOAD = re.compile(r"^global_load_dword\s")
ROW_LOAD2 = re.compile(r"^global_load_dwordx2\s")
SADDR = re.compile(r"\bs\[\d+:\d+\]")
NP = 8  # pairs of the first layer (16 rows per lane)


def late_kernel(lines, i, name, row_load=ROW_LOAD, per=4):
    """Check one late-rows kernel that starts at line i; returns (ok, next line).
    row_load / per: the row request's instruction and the requests per pair of
    rows (4 dword loads; 2 dwordx2 loads of paired rows)."""
    k = i
    marker = None
    loads_before = 0
    while not lines[k].startswith(".Lfunc_end"):
        t = lines[k].strip()
        if "late rows: prologue requested" in t:
            marker = k
            break
        if row_load.match(t):
            loads_before += 1
        k += 1
    if marker is None or loads_before % per or not 0 < loads_before <= per * NP:
        print("%-34s no prologue marker / %d row loads before it  UNEXPECTED" % (name, loads_before))
        return False, k
    D = loads_before // per
    requested = loads_before   # row loads requested so far
    done = 0                   # ... retired by the waits so far
    last = None
    wait_tab = None
    flight = []                # loads in flight at butterfly g's first v_perm
    vaddr = 0
    barrier = early_zero = False
    while not lines[k].startswith(".Lfunc_end") and len(flight) < NP:
        t = lines[k].strip()
        w = VM.search(t)
        if w:
            last = int(w.group(1))
            if last == 0 and (requested < per * NP or done < per * (NP - 1)):
                early_zero = True
            done = max(done, requested - last)
        elif row_load.match(t):
            requested += 1
            vaddr += not SADDR.search(t)
        elif t.startswith("s_barrier"):
            barrier = True
        elif t.startswith("ds_write_b128") and wait_tab is None:
            wait_tab = last
        elif t.startswith("v_perm_b32") and done >= per * (len(flight) + 1):
            # (retired past pair g + 1 before butterfly g ran: a wait too deep)
            flight.append(requested - done if done == per * (len(flight) + 1) else -1)
        k += 1
    want = [per * min(D, NP - 1 - g) for g in range(NP)]
    ok = (wait_tab is not None and wait_tab >= per * D and flight == want and requested == per * NP and not vaddr
          and not barrier and not early_zero)
    print("%-34s D %d  tables vmcnt(%s)  in flight at butterflies %s  VGPR-pair requests %d  barrier: %s  "
          "early vmcnt(0): %s  %s" % (name, D, wait_tab, ",".join(map(str, flight)), vaddr,
                                      "yes" if barrier else "no", "yes" if early_zero else "no",
                                      "ok" if ok else "UNEXPECTED (want %s)" % ",".join(map(str, want))))
    return ok, k


def main():
    lines = open(sys.argv[1]).read().splitlines()
    bad = 0
    i = 0
    while i < len(lines):
        m = LATE.match(lines[i])
        if m:
            ok, i = late_kernel(lines, i, "pass_kernel_late<%s,%s,%s>" % (NAMES[m.group(1)], m.group(2), m.group(3)))
            bad += not ok
        m = PAIRED.match(lines[i]) if i < len(lines) else None
        if m:
            name = "late_paired<%s,%s,%s,in %s,out %s>" % (NAMES[m.group(1)], m.group(2), m.group(3), m.group(4),
                                                          m.group(5))
            if m.group(4) == "1":
                ok, i = late_kernel(lines, i, name, ROW_LOAD2, 2)
            else:
                ok, i = late_kernel(lines, i, name)
            bad += not ok
        m = TOWER.match(lines[i]) if i < len(lines) else None
        if m:
            name = "late_tower<%s,%s,%s>" % (NAMES[m.group(1)], m.group(2), m.group(3))
            if m.group(1) != "2":
                ok, i = late_kernel(lines, i, name, ROW_LOAD2, 2)
            else:
                ok, i = late_kernel(lines, i, name)
            bad += not ok
        i += 1
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
