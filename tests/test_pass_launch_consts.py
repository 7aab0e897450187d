"""The pass launches' address-form decisions against an exact integer model
(CPU only: rs16_host_pass_consts evaluates the function launch_pass calls).

A pass kernel forms every HBM address as a wave-uniform row base plus a
per-lane byte offset  lane_rows x S + offL  (rs16_pass.hpp LaneOff,
request_rows, load_rows_fast, FastStore::row):

  lane_rows  rows of the lane's row set below the wave's first one: at most
             (HWS - 1) 2^R << lo in layout A, (HWS - 1) << lo in layout B
             (HWS row sets per wave, 2^R rows per thread: the hook's geometry)
  S          the row stride of the array (in / out / seg / rest)
  offL       the lane's quad within the row: the last quad's low dword at
             8 qrow - 36, its high dword 32 bytes further, 4 bytes each: the
             last byte a lane touches is at lane_rows x S + 8 qrow - 1, the
             largest dword offset  lane_rows_max x S + 8 qrow - 4

With PassArgs::voff32 the kernel keeps that offset in 32 bits; with
full_lanes it also steps row register m by m x rs_out in 32 bits (m < 16) and
takes rs_in / rs_seg / rs_out for the distance between row registers.  The
kernels trust both flags, so the test asserts, for every case:

  1. voff32 = 1  =>  the largest offset of both layouts and all four strides
     is below 2^32 (the general, the full-item and the clamped forms all use
     this offset; the clamped form's offL is not larger)
  2. full_lanes = 1  =>  voff32 = 1, qrow % quads = 0, in_rows_mask = 0,
     15 rs_out < 2^32, rs_x = S_x << (lo + the kernel's shift) with the shift
     0 (layout A) or T - R (layout B)
  3. largest offset < 2^31, chunk and row_base_in multiples of 2^(T + lo), no
     diag flag  =>  voff32 = 1: the 32-bit form is not given up for more than
     a factor 2 of slack (T = 5's predicate counts 16 rows per row set where
     the kernel has 8)
  4. RS16_DIAG_FORCE_VOFF64  =>  voff32 = 0 and full_lanes = 0

Cases: every program that has a kernel, T = 1..8, lo = 0..8; the widths 64,
1088, 2^15 +- 64, 2^16 +- 64, 2^20, 2^24; and for every (T, lo) with HWS > 1
every multiple of 64 from 512 below 2^32 / (lane_rows_max + 1) to 512 above
2^32 / lane_rows_max (layout A), the band in which the largest offset crosses
2^32.  Each as a full-width launch (all strides = 8 qrow), as a column slice
(seg / rest at the shard's stride, in / out and the slice half as wide), with
the segment boundary or the first gather row off the tile span, with a row
mask, and with the diag flag.

The sweeps run through rs16_host_pass_consts_many (the same function, one
call per sweep) and model the offsets in int64 numpy arrays: every product
is below 2^12 x 2^29, so the arithmetic is exact; the fixed widths go through
the scalar hook and Python ints.
"""
import ctypes as C

import numpy as np
import pytest

import rs16
from rs16._lib import PassConsts, lib

TWO32 = 1 << 32
FIXED_WIDTHS = (64, 1088, 2**15 - 64, 2**15 + 64, 2**16 - 64, 2**16 + 64, 2**20, 2**24)
CONSTS = np.dtype(PassConsts)


def programs():
    n = lib().rs16_prog_count()
    return [(p, lib().rs16_prog_name(p).decode()) for p in range(n)]


def consts(prog, T, lo, s_in, s_out, s_seg, s_rest, qrow, chunk=0, row_base_in=0, mask=0, diag=0):
    """The hook for one launch: PassConsts, or None when (prog, T) has no kernel."""
    out = PassConsts()
    ok = lib().rs16_host_pass_consts(prog, T, lo, s_in, s_out, s_seg, s_rest, qrow, chunk, row_base_in, mask, diag,
                                     C.byref(out))
    return out if ok else None


def consts_many(prog, T, lo, s_in, s_out, s_seg, s_rest, qrow, chunk=0, row_base_in=0, mask=0, diag=0):
    """The hook for launches that differ in strides / width: a structured array."""
    n = len(qrow)
    arrs = [np.ascontiguousarray(a, np.uint64) for a in (s_in, s_out, s_seg, s_rest)]
    q = np.ascontiguousarray(qrow, np.uint32)
    out = np.zeros(n, CONSTS)
    ok = lib().rs16_host_pass_consts_many(prog, T, lo, n, *[a.ctypes.data for a in arrs], q.ctypes.data, chunk,
                                          row_base_in, mask, diag, out.ctypes.data)
    return out if ok else None


def lane_rows_max(g, lo):
    """(layout A, layout B) from the hook's geometry."""
    hws, r = int(g["row_sets"]), int(g["reg_bits"])
    return ((hws - 1) * (1 << r)) << lo, (hws - 1) << lo


def variants(T, lo, widths):
    """(name, s_in, s_out, s_seg, s_rest, qrow, chunk, row_base_in, mask, diag) over int64 arrays of widths."""
    w = np.asarray(widths, np.int64)
    span = 1 << (T + lo)
    half = np.maximum(w // 128 * 64, 64)  # a column slice half as wide
    yield "full", w, w, w, w, w // 8, 0, 0, 0, 0
    yield "slice", half, half, w, w, half // 8, 0, 0, 0, 0
    yield "aligned-chunk", w, w, w, w, w // 8, 3 * span, span, 0, 0
    yield "chunk-off-span", w, w, w, w, w // 8, span // 2, 0, 0, 0
    yield "base-off-span", w, w, w, w, w // 8, span, span + 1, 0, 0
    yield "row-mask", w, w, w, w, w // 8, 0, 0, span - 1, 0
    yield "voff64", w, w, w, w, w // 8, 0, 0, 0, rs16.DIAG_FORCE_VOFF64


def check(T, lo, c, s_in, s_out, s_seg, s_rest, qrow, chunk, row_base_in, mask, diag, exact=False):
    """The properties over the launches of c (a structured array of the hook's
    answers); returns {property: boolean array of violations}.  exact: Python
    ints (object arrays) instead of int64."""
    if exact:
        conv = lambda a: np.array([int(x) for x in np.atleast_1d(a)], dtype=object)
    else:
        conv = lambda a: np.asarray(a, np.int64)
    s_in, s_out, s_seg, s_rest, qrow = (conv(x) for x in (s_in, s_out, s_seg, s_rest, qrow))
    g = c[0]
    get = lambda n: conv(c[n])
    B = lambda x: np.asarray(x).astype(bool)
    la, lb = lane_rows_max(g, lo)
    quads, r = int(g["quads"]), int(g["reg_bits"])
    lsh, ssh = int(g["load_shb"]), int(g["store_shb"])
    assert lsh in (0, T - r) and ssh in (0, T - r), (lsh, ssh, T, r)
    smax = np.maximum(np.maximum(s_in, s_out), np.maximum(s_seg, s_rest))
    top = max(la, lb) * smax + 8 * qrow - 4  # both layouts, all four strides
    v32, full = B(get("voff32") != 0), B(get("full_lanes") != 0)
    span = 1 << (T + lo)
    aligned = chunk % span == 0 and row_base_in % span == 0
    rs_ok = B(get("rs_in") == s_in << (lo + lsh)) & B(get("rs_seg") == s_seg << (lo + lsh)) & \
            B(get("rs_out") == s_out << (lo + ssh))
    full_ok = v32 & B(qrow % quads == 0) & (mask == 0) & B(15 * get("rs_out") < TWO32) & rs_ok
    return {
        "voff32 with an offset >= 2^32": v32 & B(top >= TWO32),
        "full_lanes without its conditions": full & ~full_ok,
        "64-bit offsets below 2^31": ~v32 & B(top < TWO32 // 2) & (aligned and diag == 0),
        "forced 64-bit offsets ignored": (v32 | full) & ((diag & rs16.DIAG_FORCE_VOFF64) != 0),
        "nslab": B(get("nslab") != (qrow + quads - 1) // quads),
    }


def report(bad, widths):
    out = []
    for what, v in bad.items():
        v = np.atleast_1d(v)
        if v.any():
            w = np.asarray(widths)[v]
            out.append(f"{what}: {len(w)} widths, {w.min()} .. {w.max()}")
    return out


def sweep_widths(la):
    first = -(-(TWO32 // (la + 1) - 512) // 64) * 64
    last = (TWO32 // la + 512) // 64 * 64
    return np.arange(first, last + 1, 64, dtype=np.int64)


@pytest.mark.parametrize("lo", range(9))
@pytest.mark.parametrize("T", range(1, 9))
def test_launch_constants(T, lo):
    failures, kernels = [], 0
    for prog, name in programs():
        g = consts(prog, T, lo, 64, 64, 64, 64, 8)
        if g is None:
            continue
        kernels += 1
        # fixed widths: Python ints through the scalar hook
        for v in variants(T, lo, FIXED_WIDTHS):
            vname, arrs, (chunk, base, mask, diag) = v[0], v[1:6], v[6:]
            c = np.zeros(len(FIXED_WIDTHS), CONSTS)
            for i in range(len(FIXED_WIDTHS)):
                one = consts(prog, T, lo, *[int(x[i]) for x in arrs], chunk, base, mask, diag)
                c[i] = tuple(getattr(one, n) for n in CONSTS.names)
            for line in report(check(T, lo, c, *arrs, chunk, base, mask, diag, exact=True), FIXED_WIDTHS):
                failures.append(f"{name} {vname}: {line}")
        # the band in which the largest offset crosses 2^32
        la, _ = lane_rows_max({"row_sets": g.row_sets, "reg_bits": g.reg_bits}, lo)
        if g.row_sets > 1:
            widths = sweep_widths(la)
            for v in variants(T, lo, widths):
                vname, arrs, (chunk, base, mask, diag) = v[0], v[1:6], v[6:]
                c = consts_many(prog, T, lo, *arrs, chunk, base, mask, diag)
                for line in report(check(T, lo, c, *arrs, chunk, base, mask, diag), widths):
                    failures.append(f"{name} {vname} sweep: {line}")
    assert kernels, "no program has a kernel at this T"
    assert not failures, "\n".join(failures)


def test_sweep_band_holds_both_answers():
    # the sweep is not vacuous: in every band the hook answers 0 at the
    # highest width, and 1 at the lowest where a row set has 16 rows (8 rows,
    # T = 5: property 3 allows the factor 2 by which its band lies higher)
    # (GEN_FFT, full-width launches)
    for T in range(1, 9):
        for lo in range(9):
            g = consts(0, T, lo, 64, 64, 64, 64, 8)
            if g.row_sets == 1:
                continue
            la, _ = lane_rows_max({"row_sets": g.row_sets, "reg_bits": g.reg_bits}, lo)
            w = sweep_widths(la)
            c = consts_many(0, T, lo, w, w, w, w, w // 8)
            assert c["voff32"][-1] == 0, (T, lo)
            assert c["voff32"][0] == 1 or g.reg_bits < 4, (T, lo)


def test_no_kernel_and_bad_arguments():
    out = PassConsts()
    f = lib().rs16_host_pass_consts
    assert f(lib().rs16_prog_count(), 6, 0, 64, 64, 64, 64, 8, 0, 0, 0, 0, C.byref(out)) == 0
    assert f(-1, 6, 0, 64, 64, 64, 64, 8, 0, 0, 0, 0, C.byref(out)) == 0
    assert f(0, 9, 0, 64, 64, 64, 64, 8, 0, 0, 0, 0, C.byref(out)) == 0
    assert f(0, 6, 0, 64, 64, 64, 64, 8, 0, 0, 0, 0, None) == 0
