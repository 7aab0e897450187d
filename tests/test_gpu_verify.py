"""rs16_verify_device / rs16_verify_device_batch (include/rs16.h): the scrub --
do the stored recovery shards still equal the encode of the stored originals,
and if not, which shards and which 64-byte column blocks differ.

Expected flags never come from the code under test.  The stored recovery is
the oracle's encode of the clean originals; after corrupting originals,
recovery or both, row flag j is any(oracle encode of the corrupted originals
[j] != stored[j]) for a checked j, and column flag c the same comparison over
bytes [64 c, 64 c + 64) of the checked rows.  Every case puts each flag array
at an odd address with 0xFF directly before and behind it, pre-fills it with
0xA5 (every byte must be written, no neighbour), puts a 64-byte guard behind
both shard arrays and checks that both, downloaded afterwards, are what was
uploaded.  The engine runs with profiling on: each case asserts which of
ENC_LAST_VFY, ENC_SINGLE_VFY and VERIFY_CMP ran, and that the other two did
not.

Shapes: one per geometry (SHAPES).  3:2, 2:3, 5:3000 and 3000:5 end their
encode in ENC_LAST at 2^1 / 2^3-row tiles, for which no comparing kernel exists
(ENC_LAST_VFY: T = 4 .. 8): they take encode + compare under every switch; 2:2,
3:4 and 5:8 are the one-pass kernel at small T.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu

GUARD = 64
NO, FORCE = rs16.DIAG_NO_FUSED_VERIFY, rs16.DIAG_FORCE_FUSED_VERIFY
NOCOL, V64 = rs16.DIAG_NO_COLUMN, rs16.DIAG_FORCE_VOFF64
VFY = ("ENC_LAST_VFY", "ENC_SINGLE_VFY", "VERIFY_CMP")
CHECK_VALUES = np.array([1, 2, 0x80, 0xFF], np.uint8)


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    e.set_profiling(True)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, sb, seed=0):
    """(clean originals, oracle recovery) of one stripe, computed once, read-only."""
    original = generate_original(k, sb, 7 * k + m + seed)
    recovery = O.encode(k, m, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def flip(a, row, byte, bit=0):
    a[row, byte] ^= np.uint8(1 << bit)


# name -> (bits to flip in the originals, in the recovery) as (row, byte, bit); byte None: the whole row 0xFF
def corruptions(k, m, sb):
    last = sb - 1
    out = {
        "none": ([], []),
        "rec_first": ([], [(0, 0, 0)]),
        "rec_last": ([], [(m - 1, last, 7)]),
        # low half (offset < 32) and high half of one 64-byte block, in different rows where there are two
        "rec_halves": ([], [(0, sb - 64 + 5, 3), (m - 1 if m > 1 else 0, sb - 64 + 37, 4)]),
        "orig_last_block": ([(k // 2, sb - 64 + 9, 1)], []),
        "both": ([(0, 1, 2), (k - 1, sb - 2, 6)], [(m // 2, min(70, last), 5)]),
        "rec_row_ff": ([], [(m // 3, None, None)]),
    }
    return out


@functools.lru_cache(maxsize=None)
def corrupted(k, m, sb, name, seed=0):
    """(stored originals, stored recovery, oracle encode of the stored originals), read-only."""
    original, recovery = stripe(k, m, sb, seed)
    co, cr = corruptions(k, m, sb)[name]
    o, r = original.copy(), recovery.copy()
    for row, byte, bit in co:
        flip(o, row, byte, bit)
    for row, byte, bit in cr:
        if byte is None:
            r[row] = 0xFF
        else:
            flip(r, row, byte, bit)
    want = O.encode(k, m, o) if co else recovery
    for a in (o, r):
        a.setflags(write=False)
    return o, r, want


def expected(stored_r, want, checked):
    """(row flags, column flags) from the oracle's encode of the stored originals."""
    diff = (stored_r != want) & (checked[:, None] != 0)
    rows = diff.any(axis=1).astype(np.uint8)
    cols = diff.reshape(diff.shape[0], -1, 64).any(axis=(0, 2)).astype(np.uint8)
    return rows, cols


def check_set(m, kind, bad_rows):
    """kind: None (NULL), 'all' (nonzero values in turn), 'skip_bad' (leaves out
    exactly the corrupted recovery rows), 'keep_one' (keeps the first of them)."""
    if kind is None:
        return None
    c = CHECK_VALUES[np.arange(m) % len(CHECK_VALUES)].copy()
    if kind in ("skip_bad", "keep_one"):
        c[bad_rows] = 0
        if kind == "keep_one" and len(bad_rows):
            c[bad_rows[0]] = 0x80
    return c


class Flags:
    """A device flag array of n bytes at an odd address, 0xFF before and behind, pre-filled 0xA5."""

    def __init__(self, eng, n, off=1, pad=3):
        self.n, self.off = n, off
        self.host = np.full(off + n + pad, 0xFF, np.uint8)
        self.host[off:off + n] = 0xA5
        self.d = DeviceArray.from_numpy(eng, self.host)
        self.ptr = self.d.ptr + off
        assert self.ptr % 2 == 1

    def read(self):
        got = self.d.download()
        assert (got[:self.off] == 0xFF).all() and (got[self.off + self.n:] == 0xFF).all(), "neighbour bytes written"
        return got[self.off:self.off + self.n]


def upload_guarded(eng, a):
    host = np.full(a.size + GUARD, 0x5A, np.uint8)
    host[:a.size] = a.reshape(-1)
    return host, DeviceArray.from_numpy(eng, host)


def run_verify(eng, k, m, sb, o, r, checked, diag, cols=True):
    """One rs16_verify_device call; returns (row flags, column flags or None, programs that ran)."""
    host_o, d_o = upload_guarded(eng, o)
    host_r, d_r = upload_guarded(eng, r)
    rows_f = Flags(eng, m)
    cols_f = Flags(eng, sb // 64, off=3) if cols else None
    d_c = None
    if checked is not None:
        cbuf = np.full(m + 2, 0xFF, np.uint8)  # odd address; 0xFF neighbours would read as "compare"
        cbuf[1:m + 1] = checked
        d_c = DeviceArray.from_numpy(eng, cbuf)
    old = eng.set_diagnostics(diag)
    try:
        eng.profile_reset()
        rs16.verify_device(k, m, sb, d_o.ptr, d_r.ptr, rows_f.ptr, cols_f.ptr if cols else None,
                           d_c.ptr + 1 if d_c else None, engine=eng)
        eng.synchronize()
        ran = {n: c for n, (ms, c) in eng.profile().items()}
    finally:
        eng.set_diagnostics(old)
    assert np.array_equal(d_o.download(), host_o), "originals (or their guard) written"
    assert np.array_equal(d_r.download(), host_r), "recovery (or its guard) written"
    return rows_f.read(), cols_f.read() if cols else None, ran


def expect_program(k, m, sb, diag):
    """The one verify id that must have launches, from the documented rule."""
    if rs16.verify_path(k, m, sb, diag=diag) != 1:
        return "VERIFY_CMP"
    high = rs16.use_high_rate(k, m)
    chunk = 1 << (m - 1).bit_length()
    return "ENC_SINGLE_VFY" if high and k <= chunk and chunk <= 256 else "ENC_LAST_VFY"


def assert_program(ran, want):
    for n in VFY:
        if n == want:
            assert ran.get(n, 0) > 0, (want, ran)
        else:
            assert ran.get(n, 0) == 0, (want, ran)


# (k, m, shard sizes, extra switches under which the shape is run as well, the
# fused program under FORCE | extra or None)
SMALL = (64, 192, 1088, 2112)
SHAPES = [
    (3, 2, SMALL, 0, None), (2, 3, SMALL, 0, None),                  # T = 1 last passes: encode + compare only
    (2, 2, (64, 192), 0, "ENC_SINGLE_VFY"), (3, 4, (64, 1088), 0, "ENC_SINGLE_VFY"),
    (5, 8, (192, 2112), 0, "ENC_SINGLE_VFY"),                        # one pass at T = 1, 2, 3
    (100, 100, SMALL, NOCOL, "ENC_SINGLE_VFY"),                      # column codec by default; one pass at T = 7
    (200, 200, (64, 192), NOCOL, "ENC_SINGLE_VFY"),                  # ... at T = 8
    (40, 200, SMALL, 0, "ENC_LAST_VFY"),                             # low rate, 4 recovery chunks, in_rows_mask, T = 6
    (5, 3000, (64, 192), 0, None), (3000, 5, (64, 192), 0, None),    # 8-row chunks
    (600, 300, (64, 192), NOCOL, "ENC_LAST_VFY"),                    # high rate, two 512-row chunks: T = 4 last pass
    (1000, 1000, (64, 192), NOCOL, "ENC_LAST_VFY"),                  # the reference's shape; T = 5
]
CASES = [(k, m, sb, extra, prog) for k, m, sbs, extra, prog in SHAPES for sb in sbs]


@pytest.mark.parametrize("k,m,sb,extra,fused_prog", CASES)
def test_small_shapes(eng, k, m, sb, extra, fused_prog):
    switch_sets = [0, NO, FORCE, FORCE | V64]
    if extra:
        switch_sets += [extra, extra | FORCE, extra | FORCE | V64]
    seen = set()
    for ci, name in enumerate(corruptions(k, m, sb)):
        o, r, want = corrupted(k, m, sb, name)
        bad = np.flatnonzero((r != stripe(k, m, sb)[1]).any(axis=1))
        kinds = [None, "all"] + (["skip_bad", "keep_one"] if len(bad) else [])
        kind = kinds[ci % len(kinds)]  # each corruption with one check set, in turn
        for kd in ([kind] if name not in ("rec_halves", "both") else kinds):
            checked = check_set(m, kd, bad)
            cm = np.ones(m, np.uint8) if checked is None else checked
            want_rows, want_cols = expected(r, want, cm)
            if name == "none":
                assert not want_rows.any() and not want_cols.any()
            if kd == "skip_bad" and not corruptions(k, m, sb)[name][0]:
                assert not want_rows.any() and not want_cols.any()  # all flags 0 although the array differs
            first = None
            for diag in switch_sets:
                rows, cols, ran = run_verify(eng, k, m, sb, o, r, checked, diag)
                assert np.array_equal(rows, want_rows), (name, kd, diag, np.flatnonzero(rows != want_rows)[:8])
                assert np.array_equal(cols, want_cols), (name, kd, diag, np.flatnonzero(cols != want_cols)[:8])
                prog = expect_program(k, m, sb, diag)
                assert_program(ran, prog)
                seen.add(prog)
                if first is None:
                    first = (rows, cols)
                assert np.array_equal(rows, first[0]) and np.array_equal(cols, first[1])
    assert "VERIFY_CMP" in seen
    if fused_prog:
        assert fused_prog in seen, seen
    else:
        assert seen == {"VERIFY_CMP"}, seen


def test_null_column_flags(eng):
    k, m, sb = 100, 100, 192
    o, r, want = corrupted(k, m, sb, "both")
    want_rows, _ = expected(r, want, np.ones(m, np.uint8))
    for diag in (0, NO, NOCOL | FORCE):
        rows, cols, ran = run_verify(eng, k, m, sb, o, r, None, diag, cols=False)
        assert cols is None and np.array_equal(rows, want_rows)
        assert_program(ran, expect_program(k, m, sb, diag))


LARGE = [(8000, 8000, 64, "ENC_LAST_VFY"), (8000, 8000, 192, "ENC_LAST_VFY"),   # T = 7
         (32768, 32768, 64, "ENC_LAST_VFY"), (32768, 32768, 1024, "ENC_LAST_VFY")]  # T = 8


@pytest.mark.parametrize("k,m,sb,fused_prog", LARGE)
def test_large_shapes(eng, k, m, sb, fused_prog):
    # two corrupted-originals variants at most (one oracle encode each): "both" and the clean originals
    for name, kinds in (("none", [None]), ("rec_halves", ["all", "skip_bad", "keep_one"]), ("rec_row_ff", [None]),
                        ("both", [None, "keep_one"])):
        o, r, want = corrupted(k, m, sb, name)
        bad = np.flatnonzero((r != stripe(k, m, sb)[1]).any(axis=1))
        for kd in kinds:
            checked = check_set(m, kd, bad)
            cm = np.ones(m, np.uint8) if checked is None else checked
            want_rows, want_cols = expected(r, want, cm)
            for diag in (0, NO, FORCE, FORCE | V64):
                rows, cols, ran = run_verify(eng, k, m, sb, o, r, checked, diag)
                assert np.array_equal(rows, want_rows), (name, kd, diag, np.flatnonzero(rows != want_rows)[:8])
                assert np.array_equal(cols, want_cols), (name, kd, diag, np.flatnonzero(cols != want_cols)[:8])
                assert_program(ran, expect_program(k, m, sb, diag))
                if diag & FORCE:
                    assert expect_program(k, m, sb, diag) == fused_prog


@pytest.mark.parametrize("k,m,sb,ns,extra", [(100, 100, 192, 5, NOCOL), (600, 300, 64, 3, NOCOL),
                                             (40, 200, 64, 2, NOCOL)])  # (the low rate, stripe by stripe)
def test_batch(eng, k, m, sb, ns, extra):
    names = ["rec_first", "none", "both", "rec_halves", "orig_last_block"][:ns]
    blocks = sb // 64
    o_stride, r_stride = k * sb + 128, m * sb + 64
    rf_stride, cf_stride = m + 7, blocks + 5
    host_o = np.full(ns * o_stride + GUARD, 0x5A, np.uint8)
    host_r = np.full(ns * r_stride + GUARD, 0x5A, np.uint8)
    stored = []
    for i, name in enumerate(names):
        o, r, want = corrupted(k, m, sb, name, seed=i)
        host_o[i * o_stride:i * o_stride + k * sb] = o.reshape(-1)
        host_r[i * r_stride:i * r_stride + m * sb] = r.reshape(-1)
        stored.append((o, r, want))
    d_o, d_r = DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, host_r)
    checked = check_set(m, "all", [])
    checked[m // 2] = 0  # one slot out of the shared check set
    d_c = DeviceArray.from_numpy(eng, checked)
    for diag in (0, NO, FORCE, extra | FORCE, extra | FORCE | V64):
        rows_f, cols_f = Flags(eng, ns * rf_stride), Flags(eng, ns * cf_stride, off=3)
        old = eng.set_diagnostics(diag)
        try:
            eng.profile_reset()
            rs16.verify_device_batch(k, m, sb, ns, d_o, o_stride, d_r, r_stride, rows_f.ptr, rf_stride, cols_f.ptr,
                                     cf_stride, d_c, engine=eng)
            eng.synchronize()
            ran = {n: c for n, (ms, c) in eng.profile().items()}
        finally:
            eng.set_diagnostics(old)
        assert_program(ran, "VERIFY_CMP" if rs16.verify_path(k, m, sb, ns, diag=diag) != 1
                       else expect_program(k, m, sb, diag))
        rows, cols = rows_f.read().reshape(ns, rf_stride), cols_f.read().reshape(ns, cf_stride)
        assert (rows[:, m:] == 0xA5).all() and (cols[:, blocks:] == 0xA5).all(), "bytes between the strides written"
        any_flag = False
        for i, (o, r, want) in enumerate(stored):
            want_rows, want_cols = expected(r, want, checked)
            assert np.array_equal(rows[i, :m], want_rows), (diag, i)
            assert np.array_equal(cols[i, :blocks], want_cols), (diag, i)
            if names[i] == "none":
                assert not want_rows.any()
            any_flag |= bool(want_rows.any())
            # the single call on the stripe alone
            r1, c1, _ = run_verify(eng, k, m, sb, o, r, checked, diag)
            assert np.array_equal(r1, rows[i, :m]) and np.array_equal(c1, cols[i, :blocks])
        assert any_flag
        assert np.array_equal(d_o.download(), host_o) and np.array_equal(d_r.download(), host_r)


def call(eng, k, m, sb, o, r, rows, cols=None, chk=None):
    err = RS16Error()
    rc = lib().rs16_verify_device(eng.h, k, m, sb, o, r, chk, rows, cols, None, C.byref(err))
    return rc, rs16.Error._from_c(err).kind if rc else None


def test_errors_in_order(eng):
    k, m, sb = 100, 100, 64
    d = DeviceArray(eng, k * sb + 128)
    f = DeviceArray(eng, 256)
    # unsupported counts come first, whatever else is wrong
    assert call(eng, 0, 4, 100, None, None, None)[1] == "UnsupportedShardCount"
    assert call(eng, 40000, 40000, sb, d.ptr, d.ptr, f.ptr)[1] == "UnsupportedShardCount"
    # then the shard size
    assert call(eng, k, m, 0, None, d.ptr + 1, None)[1] == "InvalidShardSize"
    assert call(eng, k, m, 100, None, d.ptr + 1, None)[1] == "InvalidShardSize"
    # then the arguments
    assert call(eng, k, m, sb, None, d.ptr, f.ptr)[1] == "InvalidArgument"
    assert call(eng, k, m, sb, d.ptr, None, f.ptr)[1] == "InvalidArgument"
    assert call(eng, k, m, sb, d.ptr + 32, d.ptr, f.ptr)[1] == "InvalidArgument"
    assert call(eng, k, m, sb, d.ptr, d.ptr + 16, f.ptr)[1] == "InvalidArgument"
    assert call(eng, k, m, sb, d.ptr, d.ptr, None)[1] == "InvalidArgument"
    err = RS16Error()
    b = lib().rs16_verify_device_batch

    def batch(ns, os_, rs_, rfs, cfs, cols=f.ptr + 128):
        rc = b(eng.h, k, m, sb, ns, d.ptr, os_, d.ptr, rs_, None, f.ptr, rfs, cols, cfs, None, C.byref(err))
        return rs16.Error._from_c(err).kind if rc else None

    assert batch(2, k * sb, m * sb, m - 1, 1) == "InvalidArgument"       # short row-flag stride
    assert batch(2, k * sb, m * sb, m, 0) == "InvalidArgument"           # short column-flag stride
    assert batch(2, k * sb - 64, m * sb, m, 1) == "InvalidArgument"      # short shard strides
    assert batch(2, k * sb, m * sb + 32, m, 1) == "InvalidArgument"      # ... not a multiple of 64
    assert batch((1 << 20) + 1, k * sb, m * sb, m, 1) == "InvalidArgument"
    # nstripes = 0: RS16_OK, nothing launched, nothing written
    flags = Flags(eng, m)
    eng.profile_reset()
    rc = b(eng.h, k, m, sb, 0, d.ptr, k * sb, d.ptr, m * sb, None, flags.ptr, m, None, 0, None, C.byref(err))
    eng.synchronize()
    assert rc == 0 and not eng.profile()
    assert (flags.read() == 0xA5).all()


def test_verify_keeps_decode_state(eng):
    k, m, sb = 100, 100, 192
    original, recovery = stripe(k, m, sb)
    o, r, want = corrupted(k, m, sb, "both")
    want_rows, want_cols = expected(r, want, np.ones(m, np.uint8))
    of = np.ones(k, np.uint8)
    of[[1, 50, 99]] = 0
    held = original.copy()
    held[of == 0] = 0xA5
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, recovery)
    d_fo, d_fr = DeviceArray.from_numpy(eng, of), DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    for diag in (0, NOCOL | FORCE):
        # a verify between the prepare and the prepared decode
        d_o.upload(held)
        rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, k - 3, m, engine=eng)
        rows, cols, _ = run_verify(eng, k, m, sb, o, r, None, diag)
        assert np.array_equal(rows, want_rows) and np.array_equal(cols, want_cols)
        rs16.decode_device_prepared(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
        assert np.array_equal(d_o.download(shape=(k, sb)), original)
        # a decode given a wrong count, then a verify: rs16_decode_check still reports that decode
        d_o.upload(held)
        rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 2, m, engine=eng)
        run_verify(eng, k, m, sb, o, r, None, diag)
        err = RS16Error()
        assert lib().rs16_decode_check(eng.h, None, C.byref(err)) != 0
        assert (err.v0, err.v1) == (k - 3, m)
        d_o.upload(held)
        rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 3, m, engine=eng)
        run_verify(eng, k, m, sb, o, r, None, diag)
        assert lib().rs16_decode_check(eng.h, None, C.byref(err)) == 0


def test_host_level_verify(eng):
    k, m, sb = 100, 100, 192
    o, r, want = corrupted(k, m, sb, "rec_halves")
    rows, cols = rs16.verify(k, m, list(o), list(r), engine=eng)
    assert rows.tolist() == [0, m - 1] and cols.tolist() == [sb // 64 - 1]
    rows, cols = rs16.verify(k, m, o, r, checked=[0] + [1] * (m - 1), engine=eng)
    assert rows.tolist() == [m - 1] and cols.tolist() == [sb // 64 - 1]
    rows, cols = rs16.verify(k, m, *stripe(k, m, sb), engine=eng)
    assert rows.size == 0 and cols.size == 0
