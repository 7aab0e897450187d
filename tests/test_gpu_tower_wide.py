"""The tower sequences with their first and last pass wholly in tower form
(rs16_pass.hpp pass_kernel_late_tower): ENC_FIRST
converts the caller's rows in its first layer, ENC_LAST in its last, every
layer between multiplies by three byte maps (9 lookups), and the middle pass's
one wide layer uses the c1 = 1 form.  RS16_DIAG_WIDE_TWIDDLES keeps the same
sequence and form with the 12-lookup multiply in every wide layer.  Recovery
and restored shards are the oracle's bits either way.

Shapes: those of tests/test_gpu_tower_rows.py, the smallest stripes whose
sequences take the tower form -- 16384:16384 (T = 7 / 7 / 7) and 32768:32768
(7 / 8 / 7, the wide middle layer) at 512 B (one slab of the T = 7 passes) and
1024 B (two) -- and its random stripes with their oracle results, computed once
for both files.  Every case asserts the form through the host hook.  Beside the
random rows: single-bit rows, one per bit position of an element, in the first,
a middle and the last 128-row tile of the first pass (a wrong pool entry or a
wrong column of B shows as the rows of one bit), and all-0xFF rows (every
selector at its highest value)."""
import numpy as np
import pytest

import rs16
from rs16.device import DeviceArray

from test_gpu_tower_rows import SHAPES, _encode, _engine, _forms, _stripe

gpu = pytest.mark.gpu

MULS = [pytest.param(0, id="three_maps"), pytest.param(rs16.DIAG_WIDE_TWIDDLES, id="twelve_lookups")]


def _decode(eng, k, sb, rec):
    d_o = DeviceArray.from_numpy(eng, np.full(k * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(k, np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, k, engine=eng, check=True)
    return d_o.download(shape=(k, sb)), d_r.download(shape=(k, sb))


def _check(n, sb, diag, orig, want):
    assert _forms(n, sb, n, diag) == (1, 1)
    for base in (0, n):  # the identity decode's sequence
        assert _forms(n, sb, n, diag, seg_chunk=n, base=base) == (1, 1)
    eng = _engine(diag)
    assert np.array_equal(_encode(eng, n, n, sb, orig, want), want)
    back, rec = _decode(eng, n, sb, want)
    bad = np.nonzero((back != orig).any(axis=1))[0]
    assert bad.size == 0, "rows restored wrongly: %s ..." % bad[:8]
    assert np.array_equal(rec, want)  # the recovery stays


@gpu
@pytest.mark.parametrize("diag", MULS)
@pytest.mark.parametrize("n,sb", SHAPES)
def test_random_rows(n, sb, diag):
    orig, want = _stripe(n, n, sb)
    _check(n, sb, diag, orig, want)


def _single_bit_tiles(n, sb):
    """Rows 8 bit + 3 of the 128-row tiles 0, n / 256 and n / 128 - 1 hold the element 1 << bit in every position;
    every other row is zero."""
    orig = np.zeros((n, sb // 64, 2, 32), np.uint8)
    for tile in (0, n // 256, n // 128 - 1):
        for bit in range(16):
            orig[tile * 128 + 8 * bit + 3, :, bit >> 3, :] = 1 << (bit & 7)
    return orig.reshape(n, sb)


@gpu
@pytest.mark.parametrize("diag", MULS)
@pytest.mark.parametrize("n", [16384, 32768])
def test_single_bit_rows(n, diag):
    sb = 512
    orig, want = _stripe(n, n, sb, _single_bit_tiles(n, sb), key=("bit tiles", n, sb))
    _check(n, sb, diag, orig, want)


@gpu
@pytest.mark.parametrize("diag", MULS)
@pytest.mark.parametrize("n", [16384, 32768])
def test_all_ff_rows(n, diag):
    sb = 512
    orig, want = _stripe(n, n, sb, np.full((n, sb), 0xFF, np.uint8), key=("ff", n, sb))
    _check(n, sb, diag, orig, want)
