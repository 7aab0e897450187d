"""The window / batch update's launch shape against an exact integer model of
the kernel's indexing (CPU only: rs16_host_update_batch_consts evaluates the
function launch_update_batch calls; rs16_update_batch.hip).

update_batch_kernel<N, Q, PACK> trusts six numbers of its launch: Q quads per
lane, nslab slabs of 64 Q quads per window row, rows_per_wave,
stripes_per_wave (above 1: the packed form), and a grid of `blocks` workgroups
of four waves of which `waves` have work.  With qrow = width / 8 and ngroups =
ceil(nstripes / stripes_per_wave), transcribed from the kernel in exact
integers:

  wave w            t = w / nslab, slab = w mod nslab, run = t / ngroups,
                    grp = t mod ngroups
  its rows          [r0, r1) = [run rows_per_wave, min(rows, r0 + rows_per_wave)),
                    none if r0 >= rows
  its first stripe  s0 = grp stripes_per_wave
  unpacked, lane l  stripe s0; q0 = slab 64 Q + l, idle if q0 >= qrow; column
                    c < Q is quad q0 + 64 c, or q0 once more if that lies
                    beyond the window
  packed, lane l    sl = l / qrow, q = l mod qrow; sl >= stripes_per_wave:
                    lane 0's work (sl = 0, q = 0); s0 + sl >= nstripes: the
                    group's first stripe (sl = 0, the same q); stripe s0 + sl
  quad q            the dwords at byte (q >> 3) 64 + (q & 7) 4 and 32 further

Asserted for every case of the grid:

  1. every (stripe, row, quad) of [0, nstripes) x [0, rows) x [0, qrow) is
     written by exactly one (wave, lane, column) that is not a repeat, and
     those writes cover every dword of every window row once, none beyond
  2. every other write is a repeat the kernel documents -- a column beyond the
     window on the lane's own first column, a lane of a partial group on the
     group's first stripe, a lane beyond stripes_per_wave qrow on lane 0's
     quad -- and falls where a first write of the SAME wave falls
  3. the waves with work are exactly the first `waves` waves, they fill all
     workgroups but at most three waves of the last, and each of them is
     another (run, stripe group, slab)
  4. 1 <= rows_per_wave <= 32, blocks x 256 < 2^32
  5. Q = 2 exactly when qrow >= 128 and n <= 8; the packed form exactly when
     width <= 128 and nstripes >= 2, with 64 / qrow stripes a wave
  6. one stripe gives the Q, nslab, rows_per_wave and workgroups of
     rs16_host_update_consts

A wave writes the product (its rows) x (its lanes' (stripe, quad)), so 1. is
checked as a product: the runs tile [0, rows), and the lanes of the waves of
one run write every (stripe, quad) once.
"""
from functools import lru_cache

import numpy as np
import pytest

from update_batch_ref import batch_consts
from update_ref import update_consts

TWO32 = 1 << 32
ROWS = (1, 2, 3, 31, 32, 33, 1000)
WIDTHS = (64, 128, 192, 256, 320, 448, 512, 576, 1024, 1088, 1600)
NS = (1, 8, 9, 16, 17, 32)
NSTRIPES = (1, 2, 3, 7, 8, 9, 17, 64)


@lru_cache(maxsize=None)
def lane_model(qrow, nstripes, Q, nslab, spw):
    """Failures of the lanes of the waves of one run: (grp, slab, lane, column) -> (stripe, quad)."""
    bad = []
    ngroups = -(-nstripes // spw)
    grp, slab, lane, c = np.meshgrid(np.arange(ngroups, dtype=np.int64), np.arange(nslab, dtype=np.int64),
                                     np.arange(64, dtype=np.int64), np.arange(Q, dtype=np.int64), indexing="ij")
    s0 = grp * spw
    if spw > 1:
        if Q != 1 or nslab != 1:
            return ("the packed form with several quads per lane or slabs",)
        sl, q = lane // qrow, lane % qrow
        beyond = sl >= spw
        sl, q = np.where(beyond, 0, sl), np.where(beyond, 0, q)
        short = s0 + sl >= nstripes
        sl = np.where(short, 0, sl)
        live = np.ones_like(beyond)
        first = ~beyond & ~short
        stripe, qq = s0 + sl, q
    else:
        q0 = slab * (64 * Q) + lane
        live = q0 < qrow
        q = q0 + 64 * c
        beyond = q >= qrow
        qq = np.where(beyond, q0, q)
        first = live & ~beyond
        stripe = s0
        if (c[live & beyond] < 1).any():
            bad.append("a lane's first column lies beyond the window")
    if int(s0.max()) + spw >= TWO32 or 64 * Q * nslab + 63 >= TWO32:
        bad.append("a 32-bit index overflows")
    if (stripe[live] >= nstripes).any() or (qq[live] >= qrow).any():
        bad.append("a lane works beyond the stripes or the window")
    cell = stripe * qrow + qq
    if not np.array_equal(np.bincount(cell[first], minlength=nstripes * qrow), np.ones(nstripes * qrow, np.int64)):
        bad.append("a (stripe, quad) is written by no lane or by two")
    # a repeat falls on a first write of its own wave (the same grp and slab)
    wave = grp * nslab + slab
    firsts = set(zip(wave[first].tolist(), cell[first].tolist()))
    again = live & ~first
    if not all(k in firsts for k in zip(wave[again].tolist(), cell[again].tolist())):
        bad.append("a repeated write is not a first write of the same wave")
    off = (qq[first & (stripe == 0)] >> 3) * 64 + (qq[first & (stripe == 0)] & 7) * 4
    if not np.array_equal(np.sort(np.concatenate([off, off + 32]) // 4), np.arange(2 * qrow)):
        bad.append("the writes do not cover every dword of the window row once")
    return tuple(bad)


@lru_cache(maxsize=None)
def wave_model(rows, per_run, rpw, waves, blocks):
    """Failures of the waves' (run, stripe group, slab) over the grid; per_run = nslab ngroups."""
    bad = []
    w = np.arange(4 * blocks, dtype=np.int64)
    run, rest = w // per_run, w % per_run  # (t / ngroups and (grp, slab): t = w / nslab, so run = w / (nslab ngroups))
    r0 = run * rpw
    live = r0 < rows
    if int(r0.max()) + rpw >= TWO32:
        bad.append("r0 + rows_per_wave overflows 32 bits")
    if not (live[:waves].all() and not live[waves:].any()):
        bad.append("the waves with work are not the first `waves` of the grid")
    if not 4 * (blocks - 1) < waves <= 4 * blocks:
        bad.append("the grid does not end with the last wave's workgroup")
    runs = -(-rows // rpw)
    if waves != runs * per_run or not np.array_equal(run[:waves] * per_run + rest[:waves], np.arange(waves)):
        bad.append("the waves are not one per (run, stripe group, slab)")
    r1 = np.minimum(rows, r0 + rpw)
    a, b = r0[:waves:per_run], r1[:waves:per_run]
    if not (len(a) and a[0] == 0 and b[-1] == rows and (a < b).all() and (a[1:] == b[:-1]).all()):
        bad.append("the runs do not tile [0, rows)")
    return tuple(bad)


def split_model(nslab, ngroups, waves):
    """The kernel's two divisions against wave_model's one."""
    w = np.arange(waves, dtype=np.int64)
    t = w // nslab
    slab, run, grp = w - t * nslab, t // ngroups, t % ngroups
    return np.array_equal(run, w // (nslab * ngroups)) and np.array_equal(grp * nslab + slab, w % (nslab * ngroups))


def case_failures(rows, width, n, nstripes):
    c = batch_consts(rows, width, n, nstripes)
    if c is None:
        return ["no launch"]
    qrow = width // 8
    bad = []
    if c.quads_per_lane != (2 if qrow >= 128 and n <= 8 else 1):
        bad.append(f"quads per lane {c.quads_per_lane}")
    if c.stripes_per_wave != (64 // qrow if width <= 128 and nstripes >= 2 else 1):
        bad.append(f"stripes per wave {c.stripes_per_wave}")
    if not 1 <= c.rows_per_wave <= 32:
        bad.append(f"rows per wave {c.rows_per_wave}")
    if not 0 < c.blocks * 256 < TWO32:
        bad.append(f"{c.blocks} workgroups")
    if bad or c.nslab == 0 or c.blocks > 1 << 22:
        return bad  # (nothing to model)
    ngroups = -(-nstripes // c.stripes_per_wave)
    bad += lane_model(qrow, nstripes, c.quads_per_lane, c.nslab, c.stripes_per_wave)
    bad += wave_model(rows, c.nslab * ngroups, c.rows_per_wave, c.waves, c.blocks)
    if not split_model(c.nslab, ngroups, min(c.waves, 4096)):
        bad.append("wave -> (run, stripe group, slab)")
    if nstripes == 1:
        one = update_consts(rows, width, n)
        if (c.quads_per_lane, c.nslab, c.rows_per_wave, c.blocks) != tuple(one):
            bad.append(f"one stripe: {c}, the single call: {one}")
    return bad


@pytest.mark.parametrize("n", NS)
def test_grid(n):
    failures = []
    for width in WIDTHS:
        for rows in ROWS:
            for nstripes in NSTRIPES:
                for what in case_failures(rows, width, n, nstripes):
                    failures.append(f"{rows} rows x {width} B, n = {n}, {nstripes} stripes: {what}")
    assert not failures, f"{len(failures)} failures, the first:\n" + "\n".join(failures[:20])


def test_expected_shapes():
    # (Q, slabs, rows per wave, stripes per wave, waves, workgroups)
    assert batch_consts(1000, 64, 1, 17) == (1, 1, 1, 8, 3000, 750)       # packed: 3 groups, the last of one stripe
    assert batch_consts(27, 128, 4, 5) == (1, 1, 1, 4, 54, 14)            # packed: 4 a wave, the last group of one
    assert batch_consts(27, 192, 4, 3) == (1, 1, 1, 1, 81, 21)            # unpacked from 192 bytes on
    assert batch_consts(27, 256, 4, 5) == (1, 1, 1, 1, 135, 34)
    assert batch_consts(27, 320, 4, 5) == (1, 1, 1, 1, 135, 34)
    assert batch_consts(27, 64, 4, 1) == (1, 1, 1, 1, 27, 7)              # one stripe is never packed
    assert batch_consts(1000, 1600, 8, 9) == (2, 2, 2, 1, 9000, 2250)     # two quads per lane, runs of two
    assert batch_consts(1000, 1600, 9, 9) == (1, 4, 4, 1, 9000, 2250)


def test_model_rejects_wrong_shapes():
    # the model is not vacuous: each number off by one step is seen
    rows, width, n, nstripes = 1000, 1088, 5, 9
    c = batch_consts(rows, width, n, nstripes)
    assert c == (2, 2, 2, 1, 9000, 2250) and not case_failures(rows, width, n, nstripes)
    qrow = width // 8
    assert lane_model(qrow, nstripes, 1, c.nslab, 1)              # half the columns
    assert lane_model(qrow, nstripes, 2, c.nslab - 1, 1)          # a slab short
    assert not lane_model(qrow, nstripes, 2, c.nslab + 1, 1)      # (a slab more: idle lanes only)
    per_run = c.nslab * nstripes
    assert wave_model(rows, per_run, c.rows_per_wave, c.waves, c.blocks - 1)   # the last waves have no workgroup
    assert wave_model(rows, per_run, c.rows_per_wave, c.waves, c.blocks + 1)   # an idle workgroup
    assert wave_model(rows, per_run + 1, c.rows_per_wave, c.waves, c.blocks)   # a stripe more per run
    assert wave_model(rows, per_run, c.rows_per_wave - 1, c.waves, c.blocks)   # shorter runs
    assert wave_model(rows, per_run, c.rows_per_wave, c.waves - 1, c.blocks)   # a wave with work not counted
    # packed: 7 stripes of 8 quads are one wave of 56 lanes and 8 lanes on lane 0's quad
    assert batch_consts(3, 64, 1, 7) == (1, 1, 1, 8, 3, 1) and not lane_model(8, 7, 1, 1, 8)
    assert lane_model(8, 17, 1, 1, 16)    # 16 a wave need 128 lanes
    # (the model alone, no launch has it) 24 quads: two stripes a wave and 16 lanes on lane 0's quad; a third stripe has 16 lanes only
    assert not lane_model(24, 3, 1, 1, 2) and lane_model(24, 3, 1, 1, 3)


def test_bad_arguments():
    assert batch_consts(0, 64, 1, 1) is None
    assert batch_consts(1, 0, 1, 1) is None
    assert batch_consts(1, 100, 1, 1) is None
    assert batch_consts(1, 64, 0, 1) is None
    assert batch_consts(1, 64, 33, 1) is None
    assert batch_consts(1, 64, 1, 0) is None
    assert batch_consts(1, 64, 1, 65536) is None
    assert batch_consts(1, 1 << 32, 1, 1) is None
    assert batch_consts(1, 64, 32, 1) == (1, 1, 1, 1, 1, 1)
    # the widest window and the most stripes: longer runs keep the grid below 2^32 threads
    c = batch_consts(65535, (1 << 32) - 64, 8, 65535)
    assert c is None or c.blocks * 256 < TWO32
