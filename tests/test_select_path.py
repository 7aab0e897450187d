"""The selective decode (rs16_decode_device_select, include/rs16.h) without a
device: the entry points and the host hook resolve, the Python wrappers exist,
and rs16_host_select_path answers -1 / 0 / 1 / 2 at every boundary of its
counts, at both rates and for unsupported shapes.
"""
import pytest

import rs16
from rs16._lib import lib


def test_symbols_and_wrappers():
    for name in ("rs16_decode_device_select", "rs16_decode_device_select_batch", "rs16_host_select_path"):
        assert hasattr(lib(), name), name
    for name in ("decode_device_select", "decode_device_select_batch", "select_path"):
        assert callable(getattr(rs16, name)), name
        assert name in rs16.__all__, name
    names = [lib().rs16_prog_name(p).decode() for p in range(lib().rs16_prog_count())]
    for name in ("DEC_LAST_SEL", "DEC_SINGLE_SEL", "DEC_TILE_LAST_SEL", "COL_DEC_SEL"):
        assert names.count(name) == 1, name
    # every id of the plain decode keeps its name and place
    assert names[:19] == ["GEN_FFT", "GEN_IFFT", "ENC_FIRST", "ENC_MID", "ENC_LAST", "ENC_SINGLE", "DEC_FIRST",
                          "DEC_MID", "DEC_LAST", "DEC_SINGLE", "DEC_HALF_LAST", "DEC_HALF_SINGLE", "DEC_HALF_FIRST",
                          "DEC_HALF_MID", "EVAL_POLY", "COL_ENC", "COL_DEC", "DEC_MID_DIRECT", "DEC_TILE_LAST"]
    assert len(set(names)) == len(names)


def supported(k, m):
    try:
        rs16.use_high_rate(k, m)
    except rs16.Error as e:
        assert e.kind == "UnsupportedShardCount"
        return False
    return True


def expected_path(k, m, no, nr, w):
    """The rule of include/rs16.h, written out once more."""
    if not supported(k, m) or no > k or nr > m or w > k - no or no + nr < k:
        return -1
    if no == k or w == 0:
        return 0
    return 1 if w == k - no else 2


# high rate (100:60, 32768:32768), low rate (40:200, 5:3000), the smallest shape
@pytest.mark.parametrize("k,m", [(100, 60), (40, 200), (5, 3000), (32768, 32768), (1, 1), (3, 2), (2, 3)])
def test_path_grid(k, m):
    assert supported(k, m)
    nos = sorted({0, 1, k // 2, k - 2, k - 1, k, k + 1} & set(range(k + 2)))
    nrs = sorted({0, 1, m // 2, m - 1, m, m + 1} & set(range(m + 2)))
    seen = set()
    for no in nos:
        for nr in nrs:
            lost = max(k - no, 0)
            for w in sorted({0, 1, 2, lost // 2, lost - 1, lost, lost + 1, k + 1} - {-1}):
                want = expected_path(k, m, no, nr, w)
                got = rs16.select_path(k, m, no, nr, w)
                assert got == want, (k, m, no, nr, w)
                assert lib().rs16_host_select_path(k, m, no, nr, w) == got
                seen.add(got)
    assert seen >= ({-1, 0, 1, 2} if k >= 3 else {-1, 0, 1}), seen


def test_path_boundaries():
    k, m = 100, 60
    assert rs16.select_path(k, m, k, m, 0) == 0            # everything received
    assert rs16.select_path(k, m, k, 0, 0) == 0            # ... the originals, that is
    assert rs16.select_path(k, m, k, m, 1) == -1           # wanted above the lost count (0)
    assert rs16.select_path(k, m, k - 7, m, 0) == 0        # nothing wanted
    assert rs16.select_path(k, m, k - 7, m, 1) == 2
    assert rs16.select_path(k, m, k - 7, m, 6) == 2
    assert rs16.select_path(k, m, k - 7, m, 7) == 1        # the read set covers every lost original
    assert rs16.select_path(k, m, k - 7, m, 8) == -1       # ... and one more
    assert rs16.select_path(k, m, 0, m, 1) == -1           # 60 < 100 received
    assert rs16.select_path(k, m, k - m, m, 1) == 2        # exactly original_count received
    assert rs16.select_path(k, m, k - m - 1, m, 1) == -1   # one fewer
    assert rs16.select_path(k, m, k + 1, m, 0) == -1       # counts above their shard counts
    assert rs16.select_path(k, m, k - 1, m + 1, 1) == -1
    # every original lost, one wanted: the selective decode, not the half-transform one
    assert rs16.select_path(32768, 32768, 0, 32768, 1) == 2
    assert rs16.select_path(32768, 32768, 0, 32768, 32768) == 1
    assert rs16.select_path(2, 3, 0, 3, 1) == 2


@pytest.mark.parametrize("k,m", [(0, 4), (4, 0), (40000, 40000), (65537, 1), (1, 65537), (65536, 2)])
def test_unsupported_counts(k, m):
    assert not supported(k, m)
    for no, nr, w in ((k, m, 0), (max(k - 1, 0), m, 1), (0, 0, 0)):
        assert rs16.select_path(k, m, no, nr, w) == -1
