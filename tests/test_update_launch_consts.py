"""The delta update's launch shape against an exact integer model of the
kernel's indexing (CPU only: rs16_host_update_consts evaluates the function
launch_update calls; rs16_update.hip).

update_kernel<N, Q> trusts four numbers of its launch: Q quads per lane, nslab
slabs of 64 Q quads per row, rows_per_wave, and the grid of `blocks` workgroups
of four waves.  From them (transcribed below from the kernel, all in exact
integers):

  wave w            run = w / nslab, slab = w mod nslab
  its rows          [r0, r1) = [run rows_per_wave, min(rows, r0 + rows_per_wave)),
                    none if r0 >= rows
  lane l            q0 = slab 64 Q + l, idle if q0 >= qrow
  its column c < Q  q = q0 + 64 c; a column beyond the row (q >= qrow) works on
                    q0 once more
  quad q            the dwords at byte (q >> 3) 64 + (q & 7) 4 and 32 further

Asserted for every case of the grid:

  1. every (row, quad) of [0, rows) x [0, qrow) is written by exactly one
     (wave, lane, column) that is not a repeat, and those writes cover every
     dword of every row once, none beyond the row
  2. the only other writes are a lane's columns beyond the row, which fall on
     that lane's own first column (c >= 1, q0 < qrow)
  3. no wave with work lies beyond 4 blocks (1. over the waves of the grid), and
     the last workgroup has a wave with work
  4. 1 <= rows_per_wave <= 32, blocks x 256 < 2^32
  5. Q = 2 exactly when qrow >= 128 and n <= 8, else 1
  6. the kernel's 32-bit products stay below 2^32

A wave writes the rectangle [r0, r1) x (its lanes' quads), so 1. is checked as
a product: for every slab the row intervals of its waves, sorted, tile
[0, rows) without a gap or an overlap; and the lanes of the nslab slabs write
every quad of a row once.  The model depends on the case only through
(rows, qrow) and the four numbers, so equal tuples are modelled once.
"""
from functools import lru_cache

import numpy as np
import pytest

from update_ref import update_consts

TWO32 = 1 << 32
ROWS = (list(range(1, 71)) + [8191, 8192, 8193] + list(range(16383, 16387)) + list(range(24575, 24579))
        + [32767, 32768, 61440])
SHARD_BYTES = list(range(64, 2113, 64)) + [8256, 16448, 32768, 33344, 65600]
NS = (1, 8, 9, 16, 17, 32)


@lru_cache(maxsize=None)
def quad_model(qrow, Q, nslab):
    """Failures of the lanes' columns over one row."""
    bad = []
    slab, lane, c = np.meshgrid(np.arange(nslab, dtype=np.int64), np.arange(64, dtype=np.int64),
                                np.arange(Q, dtype=np.int64), indexing="ij")
    q0 = slab * (64 * Q) + lane
    live = q0 < qrow
    q = q0 + 64 * c
    beyond = q >= qrow
    qq = np.where(beyond, q0, q)
    first, again = live & ~beyond, live & beyond
    if (64 * Q * nslab + 63) >= TWO32:
        bad.append("q0 overflows 32 bits")
    if not np.array_equal(np.bincount(qq[first], minlength=qrow), np.ones(qrow, np.int64)):
        bad.append("a quad of the row is written by no lane or by two")
    # a repeat: a column c >= 1, on the lane's own column 0 (which is a first write: q0 < qrow)
    if not ((c[again] >= 1).all() and (qq[again] == q0[again]).all() and first[..., 0][again.any(axis=2)].all()):
        bad.append("a repeated write is not the lane's own first column")
    off = (qq[first] >> 3) * 64 + (qq[first] & 7) * 4
    dwords = np.concatenate([off, off + 32]) // 4
    if not np.array_equal(np.sort(dwords), np.arange(2 * qrow)):
        bad.append("the writes do not cover every dword of the row once")
    return tuple(bad)


@lru_cache(maxsize=None)
def wave_model(rows, nslab, rpw, blocks):
    """Failures of the waves' row runs over the grid."""
    bad = []
    w = np.arange(4 * blocks, dtype=np.int64)
    run = w // nslab
    slab = w - run * nslab
    r0 = run * rpw
    live = r0 < rows
    r1 = np.minimum(rows, r0 + rpw)
    if int(r0.max()) + rpw >= TWO32:  # (idle waves compute theirs too)
        bad.append("r0 + rows_per_wave overflows 32 bits")
    if not live[-4:].any():
        bad.append("the last workgroup has no work")
    s, a, b = slab[live], r0[live], r1[live]
    order = np.lexsort((a, s))
    s, a, b = s[order], a[order], b[order]
    start = np.ones(len(s), bool)
    start[1:] = s[1:] != s[:-1]
    end = np.ones(len(s), bool)
    end[:-1] = start[1:]
    ok = (np.array_equal(s[start], np.arange(nslab)) and (a[start] == 0).all() and (b[end] == rows).all()
          and (a < b).all() and (a[1:][~start[1:]] == b[:-1][~start[1:]]).all())
    if not ok:
        bad.append("the waves' row runs do not tile [0, rows) once for every slab")
    return tuple(bad)


def case_failures(rows, S, n):
    c = update_consts(rows, S, n)
    if c is None:
        return ["no launch"]
    qrow = S // 8
    bad = []
    if c.quads_per_lane != (2 if qrow >= 128 and n <= 8 else 1):
        bad.append(f"quads per lane {c.quads_per_lane}")
    if not 1 <= c.rows_per_wave <= 32:
        bad.append(f"rows per wave {c.rows_per_wave}")
    if not 0 < c.blocks * 256 < TWO32:
        bad.append(f"{c.blocks} workgroups")
    if c.quads_per_lane not in (1, 2) or c.nslab == 0 or c.rows_per_wave == 0 or c.blocks == 0 or c.blocks > 1 << 22:
        return bad  # (nothing to model)
    bad += quad_model(qrow, c.quads_per_lane, c.nslab)
    bad += wave_model(rows, c.nslab, c.rows_per_wave, c.blocks)
    return bad


@pytest.mark.parametrize("n", NS)
def test_grid(n):
    failures = []
    for S in SHARD_BYTES:
        for rows in ROWS:
            for what in case_failures(rows, S, n):
                failures.append(f"{rows} x {S} B, n = {n}: {what}")
    assert not failures, f"{len(failures)} failures, the first:\n" + "\n".join(failures[:20])


def test_model_rejects_wrong_shapes():
    # the model is not vacuous: each number off by one step is seen
    rows, S, n = 16385, 1088, 5
    c = update_consts(rows, S, n)
    assert c == (2, 2, 4, 2049) and not case_failures(rows, S, n)
    qrow = S // 8
    assert quad_model(qrow, 1, c.nslab)            # half the columns
    assert quad_model(qrow, 2, c.nslab - 1)        # a slab short
    assert not quad_model(qrow, 2, c.nslab + 1)    # (a slab more: idle lanes only)
    assert wave_model(rows, c.nslab, c.rows_per_wave, c.blocks - 1)  # the last run has no wave
    assert wave_model(rows, c.nslab, c.rows_per_wave, c.blocks + 1)  # an idle workgroup
    assert wave_model(rows, c.nslab + 1, c.rows_per_wave, c.blocks)  # waves of another slab count
    assert wave_model(rows, c.nslab, c.rows_per_wave - 1, c.blocks)  # shorter runs


def test_wide_shards_keep_the_grid_below_2_32_threads():
    # beyond the grid: runs grow past 32 rows rather than the launch past 2^32
    # threads; checked in closed form (too many waves to enumerate)
    for S in (1 << 24, 1 << 28, (1 << 32) - 64):
        for rows in (1, 1000, 65536):
            for n in (8, 9):
                c = update_consts(rows, S, n)
                if c is None:
                    continue
                qrow = S // 8
                assert c.quads_per_lane == (2 if n <= 8 else 1)
                assert c.nslab * 64 * c.quads_per_lane >= qrow > (c.nslab - 1) * 64 * c.quads_per_lane
                runs = -(-rows // c.rows_per_wave)
                assert 4 * (c.blocks - 1) < runs * c.nslab <= 4 * c.blocks
                assert c.blocks * 256 < TWO32
    assert update_consts(65536, 1 << 24, 8) is not None


def test_bad_arguments():
    assert update_consts(0, 64, 1) is None
    assert update_consts(1, 0, 1) is None
    assert update_consts(1, 100, 1) is None
    assert update_consts(1, 64, 0) is None
    assert update_consts(1, 64, 33) is None
    assert update_consts(1, 1 << 36, 1) is None
    assert update_consts(1, 64, 32) == (1, 1, 1, 1)
