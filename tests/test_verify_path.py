"""The scrub (rs16_verify_device, include/rs16.h) without a device: the entry
points and the host hook resolve, the Python wrappers exist, the three new
profiling names sit between the decode's ids and the repair's, the two
diagnostic switches have their values, the comparing programs have kernels at
the tile sizes the engine launches them at, and rs16_host_verify_path follows
the switches.
"""
import ctypes as C

import pytest

import rs16
from rs16._lib import PassConsts, lib

NEW = ["ENC_LAST_VFY", "ENC_SINGLE_VFY", "VERIFY_CMP"]


def prog_names():
    return [lib().rs16_prog_name(p).decode() for p in range(lib().rs16_prog_count())]


def test_symbols_and_wrappers():
    for name in ("rs16_verify_device", "rs16_verify_device_batch", "rs16_host_verify_path"):
        assert hasattr(lib(), name), name
    for name in ("verify_device", "verify_device_batch", "verify"):
        assert callable(getattr(rs16, name)), name
        assert name in rs16.__all__, name
    assert callable(rs16.verify_path) and "verify_path" in rs16.__all__


def test_prog_names():
    names = prog_names()
    for name in NEW:
        assert names.count(name) == 1, name
    # every earlier id keeps its name; the decode's keep their place at the
    # front and the repair's theirs at the end (tests/test_select_path.py,
    # tests/test_repair_path.py)
    assert names[:19] == ["GEN_FFT", "GEN_IFFT", "ENC_FIRST", "ENC_MID", "ENC_LAST", "ENC_SINGLE", "DEC_FIRST",
                          "DEC_MID", "DEC_LAST", "DEC_SINGLE", "DEC_HALF_LAST", "DEC_HALF_SINGLE", "DEC_HALF_FIRST",
                          "DEC_HALF_MID", "EVAL_POLY", "COL_ENC", "COL_DEC", "DEC_MID_DIRECT", "DEC_TILE_LAST"]
    assert names[-3:] == ["DEC_LAST_ALL", "DEC_SINGLE_ALL", "REPAIR_COPY"]
    assert len(set(names)) == len(names)
    for name in NEW:
        assert 19 <= names.index(name) < len(names) - 3, name


def test_diag_constants():
    assert rs16.DIAG_NO_FUSED_VERIFY == 32768
    assert rs16.DIAG_FORCE_FUSED_VERIFY == 65536
    for name in ("DIAG_NO_FUSED_VERIFY", "DIAG_FORCE_FUSED_VERIFY"):
        assert name in rs16.__all__, name
    every = [getattr(rs16, n) for n in rs16.__all__ if n.startswith("DIAG_")]
    assert len(set(every)) == len(every) and all(v & (v - 1) == 0 for v in every)


def has_kernel(prog, T):
    out = PassConsts()
    return lib().rs16_host_pass_consts(prog, T, 0, 1024, 1024, 1024, 1024, 128, 0, 0, 0, 0, C.byref(out))


def test_kernels_exist():
    names = prog_names()
    last, single = names.index("ENC_LAST_VFY"), names.index("ENC_SINGLE_VFY")
    for T in range(4, 9):
        assert has_kernel(last, T) == 1, T
    for T in range(1, 9):
        assert has_kernel(single, T) == 1, T
    assert has_kernel(last, 3) == 0
    assert has_kernel(single, 0) == 0
    # the compare kernel is no pass program
    assert has_kernel(names.index("VERIFY_CMP"), 6) == 0
    # geometry: the comparing forms keep their encoder programs' item shapes
    for vfy, enc in ((last, names.index("ENC_LAST")), (single, names.index("ENC_SINGLE"))):
        for T in range(4, 9):
            a, b = PassConsts(), PassConsts()
            assert lib().rs16_host_pass_consts(vfy, T, 0, 1024, 1024, 1024, 1024, 128, 0, 0, 0, 0, C.byref(a)) == 1
            assert lib().rs16_host_pass_consts(enc, T, 0, 1024, 1024, 1024, 1024, 128, 0, 0, 0, 0, C.byref(b)) == 1
            for f in ("quads", "threads", "load_shb", "store_shb", "reg_bits", "row_sets", "nslab", "voff32"):
                assert getattr(a, f) == getattr(b, f), (vfy, T, f)
            assert a.late_rows == 0  # the general kernel only


# (shape, shard bytes, fused kernel exists by default switches, ... under NO_COLUMN)
SHAPES = [
    (3, 2, 64, False, False), (2, 3, 64, False, False),    # two chunks of 2 rows: the last pass at T = 1 < 4
    (1, 1, 64, False, False),                                # one-row chunk: the copy branch
    (2, 2, 64, True, True), (3, 4, 64, True, True), (5, 8, 64, True, True),  # one pass at T = 1, 2, 3
    (100, 100, 64, False, True),                             # 128-row chunk: the column codec, else one pass
    (200, 200, 64, False, True),                             # 256-row chunk: likewise
    (1000, 1000, 1024, False, True),                         # 1024-row chunk: the column codec
    (1000, 1000, 4096, True, True),                          # ... too wide for it
    (600, 300, 64, False, True), (40, 200, 64, True, True),  # multi-chunk: column forms / 64-row chunks
    (5, 3000, 64, False, False), (3000, 5, 64, False, False),  # 8-row chunks: T = 3
    (8000, 8000, 64, True, True), (32768, 32768, 1024, True, True),
]


@pytest.mark.parametrize("k,m,sb,fusable,fusable_nocol", SHAPES)
def test_path(k, m, sb, fusable, fusable_nocol):
    NO, FORCE, NOCOL = rs16.DIAG_NO_FUSED_VERIFY, rs16.DIAG_FORCE_FUSED_VERIFY, rs16.DIAG_NO_COLUMN
    assert rs16.verify_path(k, m, sb) in (0, 1)
    assert rs16.verify_path(k, m, sb, diag=NO) == 0
    assert rs16.verify_path(k, m, sb, diag=NO | FORCE) == 0
    assert rs16.verify_path(k, m, sb, diag=FORCE) == (1 if fusable else 0)
    assert rs16.verify_path(k, m, sb, diag=FORCE | NOCOL) == (1 if fusable_nocol else 0)
    # the default takes the fused path only where a kernel exists
    assert rs16.verify_path(k, m, sb) <= rs16.verify_path(k, m, sb, diag=FORCE)
    assert lib().rs16_host_verify_path(k, m, sb, 1, FORCE) == rs16.verify_path(k, m, sb, diag=FORCE)


def test_path_unsupported():
    for k, m, sb in ((0, 4, 64), (4, 0, 64), (40000, 40000, 64), (3, 2, 0), (3, 2, 100)):
        assert rs16.verify_path(k, m, sb) == -1
        assert rs16.verify_path(k, m, sb, diag=rs16.DIAG_FORCE_FUSED_VERIFY) == -1


def test_default_gate():
    """The default is the fused path only for batches of the one-chunk high rate
    at 1024-row chunks that the pass codec encodes (include/rs16.h, "When to
    prefer it")."""
    for ns in (4, 8, 32, 1000):
        assert rs16.verify_path(1000, 1000, 1024, ns) == 1, ns
    assert rs16.verify_path(600, 1024, 4096, 4) == 1
    assert rs16.verify_path(1000, 1000, 64, 4) == 0        # 32 quad columns: the column codec encodes the batch
    assert rs16.verify_path(1000, 1000, 64, 4, diag=rs16.DIAG_NO_COLUMN) == 1
    assert rs16.verify_path(1000, 1000, 1024, 32, diag=rs16.DIAG_NO_FUSED_VERIFY) == 0
    for k, m, sb, ns in ((1000, 1000, 1024, 1), (1000, 1000, 4096, 1), (1000, 1000, 4096, 3), (32768, 32768, 1024, 1),
                         (8000, 8000, 1024, 1), (8000, 8000, 1024, 8), (60000, 3000, 1024, 1), (500, 500, 4096, 8),
                         (2000, 2000, 1024, 8), (40, 200, 64, 8), (100, 100, 64, 8)):
        assert rs16.verify_path(k, m, sb, ns) == 0, (k, m, sb, ns)
    assert rs16.verify_path(1000, 1000, 1024, diag=rs16.DIAG_NO_COLUMN) == 0
    assert rs16.verify_path(1000, 1000, 1024, diag=rs16.DIAG_NO_COLUMN | rs16.DIAG_FORCE_FUSED_VERIFY) == 1
