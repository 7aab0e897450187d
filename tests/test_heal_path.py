"""The heal and the batch locate (include/rs16.h "Heal") without a device: the
entry points and the host hook resolve, the Python wrappers exist, the heal's
mask constants have their values, the new profiling name sits between the
decode's ids and the repair's, and the scan launch's shape
(rs16_host_locate_scan_shape) holds its invariants for every stripe count and
is, for one stripe, what it was before the stripe dimension.
"""
import ctypes as C
import itertools

import pytest

import rs16
from rs16._lib import lib

SYMBOLS = ["rs16_locate_device_batch", "rs16_heal_device", "rs16_heal_device_batch", "rs16_host_locate_scan_shape"]
WRAPPERS = ["locate_device_batch", "heal_device", "heal_device_batch", "heal", "HEAL_ORIGINAL", "HEAL_RECOVERY"]


def prog_names():
    return [lib().rs16_prog_name(p).decode() for p in range(lib().rs16_prog_count())]


def scan_shape(S, m, n):
    out = (C.c_uint32 * 5)()
    rc = lib().rs16_host_locate_scan_shape(S, m, n, out)
    return None if rc else tuple(out)


def test_symbols_and_wrappers():
    for name in SYMBOLS + ["rs16_locate_device"]:
        assert getattr(lib(), name) is not None, name
    for name in WRAPPERS:
        assert hasattr(rs16, name), name
        assert name in rs16.__all__, name
    for name in ("locate_batch", "heal", "heal_batch"):
        assert callable(getattr(rs16.LocatePlan, name)), name
    assert (rs16.HEAL_ORIGINAL, rs16.HEAL_RECOVERY) == (1, 2)
    assert rs16.locate_scan_shape(64, 3) == scan_shape(64, 3, 1)


def test_prog_names():
    names = prog_names()
    assert names.count("LOCATE_APPLY") == 1
    assert names[:19] == ["GEN_FFT", "GEN_IFFT", "ENC_FIRST", "ENC_MID", "ENC_LAST", "ENC_SINGLE", "DEC_FIRST",
                          "DEC_MID", "DEC_LAST", "DEC_SINGLE", "DEC_HALF_LAST", "DEC_HALF_SINGLE", "DEC_HALF_FIRST",
                          "DEC_HALF_MID", "EVAL_POLY", "COL_ENC", "COL_DEC", "DEC_MID_DIRECT", "DEC_TILE_LAST"]
    assert names[-3:] == ["DEC_LAST_ALL", "DEC_SINGLE_ALL", "REPAIR_COPY"]
    assert len(set(names)) == len(names)
    assert 19 <= names.index("LOCATE_APPLY") < len(names) - 3
    # behind the locate's three, which keep their order
    at = names.index("LOCATE_SCAN")
    assert names[at:at + 4] == ["LOCATE_SCAN", "LOCATE_DECIDE", "LOCATE_CONFIRM", "LOCATE_APPLY"]


SIZES = [64, 128, 192, 256, 512, 1024, 1088, 2048, 2112, 4096, 8192, 16384, 32768, 65536, 65600, 131072]
ROWS = [2, 3, 1000, 32768, 65535]
STRIPES = [1, 3, 300, 2500, 65535]
SCAN_WGS = 2048  # the workgroups a scan launch aims at


def test_scan_shape_invariants():
    for S, m, n in itertools.product(SIZES, ROWS, STRIPES):
        sh = scan_shape(S, m, n)
        assert sh is not None, (S, m, n)
        cw, rsub, gx, gy, rows_per_wg = sh
        assert cw >= 1 and rsub >= 1 and cw * rsub <= 256, (S, m, n, sh)
        assert gx * cw >= S // 8, (S, m, n, sh)
        assert gy >= 1, (S, m, n, sh)
        assert gy * rows_per_wg >= m, (S, m, n, sh)
        assert rows_per_wg % rsub == 0, (S, m, n, sh)
        # what does not depend on the stripes
        assert sh[:3] == scan_shape(S, m, 1)[:3], (S, m, n, sh)
        # about SCAN_WGS workgroups in all: one row chunk once the columns and stripes alone exceed it
        if gx * n > SCAN_WGS:
            assert gy == 1, (S, m, n, sh)
        else:
            assert gx * n * gy <= SCAN_WGS, (S, m, n, sh)
        assert gy <= scan_shape(S, m, 1)[3], (S, m, n, sh)


@pytest.mark.parametrize("S,m,want", [(64, 3, (8, 32, 1, 1, 32)), (1024, 32768, (128, 2, 1, 2048, 16)),
                                      (1088, 1000, (136, 1, 1, 250, 4)), (2112, 3, (256, 1, 2, 1, 3)),
                                      (65600, 5, (256, 1, 33, 2, 3))])
def test_scan_shape_of_one_stripe_is_unchanged(S, m, want):
    """Derived by hand from locate_scan_shape as it was before it took a stripe
    count (cols = S / 8 lanes; 256 or cols of them per workgroup; at most 2048
    / gx row chunks, every thread at least four rows, chunks rounded up to rsub)."""
    assert scan_shape(S, m, 1) == want


def test_scan_shape_rejects():
    for S, m, n in [(0, 3, 1), (100, 3, 1), (64, 0, 1), (64, 65536, 1), (64, 3, 0), (64, 3, 65536), (2**32, 3, 1)]:
        assert scan_shape(S, m, n) is None, (S, m, n)
    assert lib().rs16_host_locate_scan_shape(64, 3, 1, None) != 0
