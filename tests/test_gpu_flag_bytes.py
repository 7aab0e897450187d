"""The received-flag contract of include/rs16.h through every flag reader: a
flag byte means "received" when it is NONZERO (1, 2, 0x40, 0x80, 0xFF ...),
flag arrays need no alignment, and no byte before or behind a flag array is
read as a flag.  Every other GPU test uploads flags of 0 and 1 only.

The device and the host read the caller's flag bytes in a dozen separately
written places (rs16_eval.hip: erasure_at / received_at, nz80 + sdot4 in
eval_fused_kernel, eval_small_kernel; rs16_col.hip: ColEval::prep and the
gathers of col_kernel / col2_kernel; rs16_pass.hpp: RcvCount; the reveal's
row_lost_original in rs16_pass_common.hpp; rs16_api_host.cpp: the host counts,
copy_runs; rs16_api.cpp: the flags-only count of rs16_decode_check).  A reader
written as `& 1`, `== 1`, a signed `> 0` or a byte sum restores wrong data for a caller
whose "true" is not 1; the cases below are the smallest shapes that reach
each reader (DESIGN.md 3.11, rs16_engine::decode_eval), with flags "dressed"
in a palette of nonzero values.

Every case
  - keeps its flag arrays inside a device buffer of 0xFF: the byte before the
    first flag and every byte behind the last say "received"; the originals'
    flags start at byte `off` (0: 16-byte aligned, the one-kernel eval form
    where the geometry allows it; 3: the two-kernel form), the recovery flags
    at the same residue behind a gap;
  - gives the decode exactly the shards it needs (received originals +
    received recovery == k, asserted by make_masks): a reader that drops a
    received row cannot hide behind surplus shards, one that invents a row
    changes the erasure set;
  - takes its recovery from rs16.encode_device (its parity with the oracle is
    the business of other files) and expects the original data bit for bit,
    the received originals untouched, the recovery array and the flag buffer
    unchanged; lost original slots hold 0xA5, unreceived recovery slots 0x3C;
  - runs rs16_decode_check (check=True) wherever the entry point has it, so
    the device's received counts are compared with the number of nonzero
    bytes too.

The second half pins the alignment rule of device shard arrays (64 bytes,
include/rs16.h "Conventions"): misaligned bases are refused by the C wrappers
without a launch, and a base = 64 (mod 128) works."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu

PALETTE = (0x01, 0x02, 0x40, 0x7F, 0x80, 0xAA, 0xFE, 0xFF)
SB = 64
NC, FULL, R4 = rs16.DIAG_NO_COLUMN, rs16.DIAG_EVAL_FULL, rs16.DIAG_COL_RADIX4
NOID = rs16.DIAG_NO_IDENTITY


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


def dress(mask, seed, value=None):
    """uint8 flags of a received mask: 0 where it is false, PALETTE[(7 i + seed)
    % 8] at row i where it is true (deterministic; 7 is a unit mod 8, so any
    eight consecutive received rows carry all eight values).  value: every
    received byte that value (the uniform variants)."""
    mask = np.asarray(mask, bool)
    pal = np.array(PALETTE, np.uint8)[(7 * np.arange(mask.size) + seed) % 8]
    if value is not None:
        pal = np.full(mask.size, value, np.uint8)
    return np.where(mask, pal, 0).astype(np.uint8)


def make_masks(k, m, loss, seed):
    """(originals received, recovery received) with exactly k received rows."""
    rng = np.random.default_rng(seed)
    om = np.ones(k, bool)
    if loss == "half":
        om[rng.choice(k, min(k, m) // 2, replace=False)] = False
    elif loss == "third":
        om[rng.choice(k, min(k, m) // 3, replace=False)] = False
    elif loss in ("tail", "tail_first"):
        om[k - max(1, k // 100):] = False
    elif loss == "all":
        om[:] = False
    else:
        assert loss == "none", loss
    nlost = int((~om).sum())
    assert nlost <= m
    rm = np.zeros(m, bool)
    if loss == "tail_first":
        rm[:nlost] = True  # the first recovery shards
    else:
        rm[rng.choice(m, nlost, replace=False)] = True
    # the condition of this file: no surplus shard
    assert int(om.sum()) + int(rm.sum()) == k
    return om, rm


_STRIPES = {}


def stripe(eng, k, m, sb=SB, tag=0):
    """(original, recovery) of one k:m stripe, computed once (the shipped
    encode) and shared read-only.  tag: another stripe of the same shape."""
    key = (k, m, sb, tag)
    if key not in _STRIPES:
        original = generate_original(k, sb, (31 * k + m + 7 * tag) % 251).copy()
        d_o, d_r = DeviceArray.from_numpy(eng, original), DeviceArray(eng, m * sb)
        old = eng.set_diagnostics(0)
        try:
            rs16.encode_device(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
        finally:
            eng.set_diagnostics(old)
        recovery = d_r.download(shape=(m, sb)).copy()
        original.setflags(write=False)
        recovery.setflags(write=False)
        _STRIPES[key] = (original, recovery)
    return _STRIPES[key]


def flag_buffer(fo, fr, off):
    """Both flag arrays inside 0xFF: (buffer, offset of fo, offset of fr); the
    two offsets have the same residue mod 16."""
    ro = off + (fo.size // 16 + 2) * 16
    buf = np.full(ro + fr.size + 64, 0xFF, np.uint8)
    buf[off:off + fo.size] = fo
    buf[ro:ro + fr.size] = fr
    return buf, off, ro


def holes(original, om):
    held = original.copy()
    held[~om] = 0xA5
    return held


def given(recovery, rm):
    rec = recovery.copy()
    rec[~rm] = 0x3C
    return rec


def same(got, want, what):
    bad = np.flatnonzero((got != want).reshape(got.shape[0], -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.shape[0]} rows differ, first {bad[:8].tolist()}"


def decode_case(eng, k, m, loss, off, diag=0, value=None, seed=1, sb=SB, prepared=False):
    original, recovery = stripe(eng, k, m, sb)
    om, rm = make_masks(k, m, loss, seed + k + m)
    buf, oo, ro = flag_buffer(dress(om, seed, value), dress(rm, seed + 3, value), off)
    rec = given(recovery, rm)
    d_x = DeviceArray.from_numpy(eng, holes(original, om))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_f = DeviceArray.from_numpy(eng, buf)
    assert d_f.ptr % 16 == 0 and d_x.ptr % 64 == 0 and d_r.ptr % 64 == 0
    no, nr = int(om.sum()), int(rm.sum())
    old = eng.set_diagnostics(diag)
    try:
        if prepared:
            side = eng.create_stream()
            try:
                rs16.decode_prepare(k, m, sb, d_f.ptr + oo, d_f.ptr + ro, no, nr, stream=side, engine=eng)
                rs16.decode_device_prepared(k, m, sb, d_x.ptr, d_r.ptr, engine=eng, check=True)
            finally:
                eng.synchronize()
                eng.synchronize(side)
                eng.destroy_stream(side)
        else:
            rs16.decode_device(k, m, sb, d_x.ptr, d_f.ptr + oo, d_r.ptr, d_f.ptr + ro, no, nr, engine=eng,
                               check=True)
    finally:
        eng.set_diagnostics(old)
    same(d_x.download(shape=(k, sb)), original, "originals")
    same(d_r.download(shape=(m, sb)), rec, "recovery")
    assert np.array_equal(d_f.download(), buf), "flag buffer"


def test_dress():
    m = np.ones(64, bool)
    m[::5] = False
    for seed in range(8):
        f = dress(m, seed)
        assert f.dtype == np.uint8 and (f[~m] == 0).all() and (f[m] != 0).all()
        full = dress(np.ones(64, bool), seed)
        for i in range(64 - 7):
            w = full[i:i + 8]
            assert sorted(w.tolist()) == sorted(PALETTE)  # an even value, one >= 0x80, 0xFF ... in any 8 rows
    assert (dress(m, 0, 0x80)[m] == 0x80).all() and (dress(m, 0, 0x02)[~m] == 0).all()
    assert all(v != 1 for v in PALETTE[1:])


# reader reached: (k, m, diag, loss, off, uniform value)
DEVICE_CASES = {
    # eval_small_kernel + the pass codec's reveal (three passes at 1024 work rows, DEC_SINGLE at 256)
    "small-300-half-0": (300, 300, NC, "half", 0, None),
    "small-300-half-3": (300, 300, NC, "half", 3, None),
    "small-300-tail-0": (300, 300, NC, "tail", 0, None),
    "small-300-tail-3": (300, 300, NC, "tail", 3, None),
    "small-300-all-3": (300, 300, NC, "all", 3, None),      # pass half decode, 512-row half
    "single-100-half-0": (100, 100, NC, "half", 0, None),
    "single-100-half-3": (100, 100, NC, "half", 3, None),
    "single-100-tail-0": (100, 100, NC, "tail", 0, None),
    "single-100-tail-3": (100, 100, NC, "tail", 3, None),
    "single-100-all-0": (100, 100, NC, "all", 0, None),     # DEC_HALF_SINGLE
    # the full-size eval at n <= 2048 (unaligned segments: two-kernel form)
    "full-300-half-0": (300, 300, NC | FULL, "half", 0, None),
    "full-300-half-3": (300, 300, NC | FULL, "half", 3, None),
    # eval_fused_kernel: nz80 + sdot4 (aligned flags, 256-row segments)
    "fused-2048-half": (2048, 2048, 0, "half", 0, None),
    "fused-2048-half-0x80": (2048, 2048, 0, "half", 0, 0x80),
    "fused-2048-half-0x02": (2048, 2048, 0, "half", 0, 0x02),
    "fused-2048-all": (2048, 2048, NOID, "all", 0, None),
    "fused-2048-all-0x80": (2048, 2048, NOID, "all", 0, 0x80),
    "fused-2048-all-0x02": (2048, 2048, NOID, "all", 0, 0x02),
    # the two-kernel form: erasure_at / received_at
    "two-2048-half-3": (2048, 2048, 0, "half", 3, None),
    "two-2048-tail-3": (2048, 2048, 0, "tail", 3, None),
    "two-2048-all-3": (2048, 2048, NOID, "all", 3, None),
    "two-2000-half-0": (2000, 2000, 0, "half", 0, None),    # segments that are no whole 256-row blocks
    "two-2000-tail-0": (2000, 2000, 0, "tail", 0, None),
    # RcvCount: the identity decode runs no eval kernel, its passes count the flags
    "ident-2048-0": (2048, 2048, 0, "all", 0, None),
    "ident-2048-3": (2048, 2048, 0, "all", 3, None),
    "ident-2048-0x80": (2048, 2048, 0, "all", 0, 0x80),
    # low rate: the originals are segment A
    "low-300:3000-0": (300, 3000, 0, "third", 0, None),
    "low-300:3000-3": (300, 3000, 0, "third", 3, None),
    "low-100:1000-0": (100, 1000, 0, "third", 0, None),     # column general decode
    "low-100:1000-3": (100, 1000, 0, "third", 3, None),
    # ColEval::prep + col2_kernel's gather (general decode and all lost)
    "col-300-half-0": (300, 300, 0, "half", 0, None),
    "col-300-half-3": (300, 300, 0, "half", 3, None),
    "col-300-all-0": (300, 300, 0, "all", 0, None),
    "col-300-all-3": (300, 300, 0, "all", 3, None),
    "col-100-half-0": (100, 100, 0, "half", 0, None),
    "col-100-half-3": (100, 100, 0, "half", 3, None),
    "col-100-all-0": (100, 100, 0, "all", 0, None),
    "col-100-all-3": (100, 100, 0, "all", 3, None),
    # col_kernel (radix-4)
    "r4-300-half-0": (300, 300, R4, "half", 0, None),
    "r4-300-half-3": (300, 300, R4, "half", 3, None),
    "r4-300-all-0": (300, 300, R4, "all", 0, None),
    "r4-300-all-3": (300, 300, R4, "all", 3, None),
    "r4-100-half-0": (100, 100, R4, "half", 0, None),
    "r4-100-half-3": (100, 100, R4, "half", 3, None),
    "r4-100-all-0": (100, 100, R4, "all", 0, None),
    "r4-100-all-3": (100, 100, R4, "all", 3, None),
    "r4-50:60-half-0": (50, 60, 0, "half", 0, None),        # 128 work rows: radix-4 as shipped
    "r4-50:60-half-3": (50, 60, 0, "half", 3, None),
    "r4-50:60-all-0": (50, 60, 0, "all", 0, None),
    "r4-50:60-all-3": (50, 60, 0, "all", 3, None),
    # the 65536-row metadata: lostpart / lostrange, zflags, mid_direct, tile_last
    "big-32768-0": (32768, 32768, 0, "tail_first", 0, None),
    "big-32768-3": (32768, 32768, 0, "tail_first", 3, None),
}


@pytest.mark.parametrize("case", list(DEVICE_CASES))
def test_decode_device(eng, case):
    k, m, diag, loss, off, value = DEVICE_CASES[case]
    decode_case(eng, k, m, loss, off, diag=diag, value=value)


@pytest.mark.parametrize("off", [0, 3])
def test_prepared(eng, off):
    decode_case(eng, 4096, 4096, "half", off, prepared=True)


def decode_check(eng):
    """rs16_decode_check of the engine's last decode: (rc, code, v0, v1)."""
    err = RS16Error()
    rc = lib().rs16_decode_check(eng.h, None, C.byref(err))
    return rc, err.code, err.v0, err.v1


@pytest.mark.parametrize("off", [0, 3])
def test_shared_batch(eng, off):
    k = m = 300
    n, pad = 3, 64
    so, sr = k * SB + pad, m * SB + pad
    om, rm = make_masks(k, m, "half", 17)
    orig, recs = zip(*(stripe(eng, k, m, tag=i) for i in range(n)))  # three stripes, one pattern
    host_o = np.full(n * so, 0x3C, np.uint8)
    host_r = np.full(n * sr, 0x3C, np.uint8)
    for i in range(n):
        host_o[i * so:i * so + k * SB] = holes(orig[i], om).reshape(-1)
        host_r[i * sr:i * sr + m * SB] = given(recs[i], rm).reshape(-1)
    buf, oo, ro = flag_buffer(dress(om, 2), dress(rm, 6), off)
    d_x, d_r, d_f = (DeviceArray.from_numpy(eng, a) for a in (host_o, host_r, buf))
    rs16.decode_device_batch(k, m, SB, n, d_x.ptr, so, d_f.ptr + oo, d_r.ptr, sr, d_f.ptr + ro, int(om.sum()),
                             int(rm.sum()), engine=eng)
    assert decode_check(eng) == (0, 0, 0, 0)
    got = d_x.download()
    for i in range(n):
        same(got[i * so:i * so + k * SB].reshape(k, SB), orig[i], f"stripe {i}")
        assert (got[i * so + k * SB:(i + 1) * so] == 0x3C).all(), i
    assert np.array_equal(d_r.download(), host_r)
    assert np.array_equal(d_f.download(), buf)


@pytest.mark.parametrize("k,n,off", [(300, 3, 0), (300, 3, 3), (4096, 2, 0), (4096, 2, 3)])
def test_varied_batch(eng, k, n, off):
    # per-stripe flags, each stripe a loss of its own (one loses nothing), the
    # flag strides padded with 0xFF; 4096 at off 0 keeps both strides multiples
    # of 16, so the one-kernel eval form runs with a grid row per stripe
    m, pad = k, 64
    so, sr = k * SB + pad, m * SB + pad
    data = [stripe(eng, k, m, tag=i) for i in range(n)]
    losses = ["half", "none", "tail"] if n == 3 else ["none", "half"]
    masks = [make_masks(k, m, loss, 23 + i) for i, loss in enumerate(losses)]
    fso, fsr = (k + 16, m + 32) if k == 4096 else (k + 3, m + 5)
    ro = off + ((n * fso) // 16 + 2) * 16
    buf = np.full(ro + n * fsr + 64, 0xFF, np.uint8)
    host_o = np.full(n * so, 0x3C, np.uint8)
    host_r = np.full(n * sr, 0x3C, np.uint8)
    for i, (om, rm) in enumerate(masks):
        buf[off + i * fso:off + i * fso + k] = dress(om, i)
        buf[ro + i * fsr:ro + i * fsr + m] = dress(rm, i + 4)
        host_o[i * so:i * so + k * SB] = holes(data[i][0], om).reshape(-1)
        host_r[i * sr:i * sr + m * SB] = given(data[i][1], rm).reshape(-1)
    d_x, d_r, d_f = (DeviceArray.from_numpy(eng, a) for a in (host_o, host_r, buf))
    assert d_f.ptr % 16 == 0
    rs16.decode_device_batch_varied(k, m, SB, n, d_x.ptr, so, d_f.ptr + off, fso, d_r.ptr, sr, d_f.ptr + ro, fsr,
                                    [int(om.sum()) for om, _ in masks], [int(rm.sum()) for _, rm in masks],
                                    engine=eng)
    got = d_x.download()
    for i in range(n):
        same(got[i * so:i * so + k * SB].reshape(k, SB), data[i][0], f"stripe {i}")
        assert (got[i * so + k * SB:(i + 1) * so] == 0x3C).all(), i
    assert np.array_equal(d_r.download(), host_r)
    assert np.array_equal(d_f.download(), buf)


def host_flags(fo, fr, off):
    """Host flag arrays inside one 0xFF buffer (views of it)."""
    buf, oo, ro = flag_buffer(fo, fr, off)
    return buf, buf[oo:oo + fo.size], buf[ro:ro + fr.size]


@pytest.mark.parametrize("off", [0, 3])
def test_decode_host(eng, off):
    # the host count of rs16_decode_host, then the raw bytes on the device
    # (a stripe of its own per case: the engine's staging rows keep the bytes
    # of the previous call, and a row that wrongly stays behind must not find
    # its own data there)
    k, m, sb = 1000, 1000, 128
    original, recovery = stripe(eng, k, m, sb, tag=off)
    om, rm = make_masks(k, m, "third", 5)
    buf, fo, fr = host_flags(dress(om, 1), dress(rm, 4), off)
    keep = buf.copy()
    x, rec = holes(original, om), given(recovery, rm)
    want_rec = rec.copy()
    rs16.decode_host(k, m, sb, x, fo, rec, fr, slice_bytes=64, engine=eng)
    same(x, original, "originals")
    assert np.array_equal(rec, want_rec) and np.array_equal(buf, keep)


@pytest.mark.parametrize("off", [0, 3])
def test_decode_host_batch(eng, off):
    # copy_runs selects the rows that travel, run by run up to 64 runs and as
    # one span beyond: isolated losses (60 and 33 single rows: as many runs of
    # lost rows, one more of received ones, 60 / 33 of received recovery rows)
    # go run by run, a third lost at random (more than 64 runs) as spans.
    # Every stripe has data of its own: the lanes' device rows keep the
    # previous stripe's bytes, and a row that wrongly stays behind must not
    # find its own data there.
    k = m = 300
    n = 3
    data = [stripe(eng, k, m, tag=3 + i + 3 * off) for i in range(n)]

    def isolated(nlost, seed):
        rng = np.random.default_rng(seed)
        om, rm = np.ones(k, bool), np.zeros(m, bool)
        om[2 * rng.choice(k // 2, nlost, replace=False)] = False
        rm[2 * rng.choice(m // 2, nlost, replace=False) + 1] = True
        assert int(om.sum()) + int(rm.sum()) == k
        return om, rm

    masks = [isolated(60, 40), isolated(33, 41), make_masks(k, m, "third", 42)]
    fso, fsr = k + 3, m + 5
    ro = off + ((n * fso) // 16 + 2) * 16
    buf = np.full(ro + n * fsr + 64, 0xFF, np.uint8)
    xs = np.empty((n, k, SB), np.uint8)
    recs = np.empty((n, m, SB), np.uint8)
    for i, (om, rm) in enumerate(masks):
        buf[off + i * fso:off + i * fso + k] = dress(om, i + 1)
        buf[ro + i * fsr:ro + i * fsr + m] = dress(rm, i + 5)
        xs[i], recs[i] = holes(data[i][0], om), given(data[i][1], rm)
    keep, want_recs = buf.copy(), recs.copy()
    rs16.decode_host_batch(k, m, SB, n, xs, k * SB, buf[off:], fso, recs, m * SB, buf[ro:], fsr, engine=eng)
    for i in range(n):
        same(xs[i], data[i][0], f"stripe {i}")
    assert np.array_equal(recs, want_recs) and np.array_equal(buf, keep)


def test_decode_host_multi(eng):
    k, m, sb = 1000, 1000, 128
    original, recovery = stripe(eng, k, m, sb, tag=5)
    om, rm = make_masks(k, m, "third", 9)
    buf, fo, fr = host_flags(dress(om, 6), dress(rm, 2), 3)
    x, rec = holes(original, om), given(recovery, rm)
    second = rs16.Engine(0)
    try:
        rs16.decode_host_multi(k, m, sb, x, fo, rec, fr, [eng, second])
    finally:
        second.close()
    same(x, original, "originals")


@pytest.mark.parametrize("off", [0, 3])
def test_nothing_to_restore(eng, off):
    # every original received: no kernel reads the flags, rs16_decode_check
    # counts a copy of them (note_flags_only) -- nonzero bytes, not their sum.
    # (The one case with surplus shards: nothing is decoded.)
    k = m = 300
    original, recovery = stripe(eng, k, m)
    om = np.ones(k, bool)
    rm = np.zeros(m, bool)
    rm[[0, 7, 8, 150, m - 1]] = True
    buf, oo, ro = flag_buffer(dress(om, 3), dress(rm, 1), off)
    d_x, d_r, d_f = (DeviceArray.from_numpy(eng, a) for a in (original, given(recovery, rm), buf))
    rs16.decode_device(k, m, SB, d_x.ptr, d_f.ptr + oo, d_r.ptr, d_f.ptr + ro, k, 5, engine=eng, check=True)
    same(d_x.download(shape=(k, SB)), original, "originals")
    # and through a preparation
    rs16.decode_prepare(k, m, SB, d_f.ptr + oo, d_f.ptr + ro, k, 5, engine=eng)
    rs16.decode_device_prepared(k, m, SB, d_x.ptr, d_r.ptr, engine=eng, check=True)


@pytest.mark.parametrize("k,value", [(2048, None), (2048, 0x02), (300, None), (300, 0x02)],
                         ids=["identity-2048", "identity-2048-0x02", "column-300", "column-300-0x02"])
def test_checked_mode_counts_nonzero_bytes(eng, k, value):
    # tests/test_gpu_identity.py::test_checked_mode_catches_a_missing_recovery_flag
    # with dressed flags: the counts claim every recovery shard, the flags miss
    # one.  The check must fail with the NUMBER of nonzero bytes (0 originals,
    # m - 1 recovery shards), whatever their values.  2048: the identity
    # decode's passes count (RcvCount); 300: the column codec's ColEval::prep.
    m = k
    original, recovery = stripe(eng, k, m)
    rm = np.ones(m, bool)
    rm[m // 3] = False
    buf, oo, ro = flag_buffer(dress(np.zeros(k, bool), 0), dress(rm, 5, value), 0)
    d_x = DeviceArray.from_numpy(eng, np.full((k, SB), 0xA5, np.uint8))
    d_r, d_f = DeviceArray.from_numpy(eng, recovery), DeviceArray.from_numpy(eng, buf)
    rs16.decode_device(k, m, SB, d_x.ptr, d_f.ptr + oo, d_r.ptr, d_f.ptr + ro, 0, m, engine=eng)
    assert decode_check(eng) == (101, 101, 0, m - 1)  # RS16_INVALID_ARGUMENT, v0 originals, v1 recovery
    with pytest.raises(rs16.Error) as e:
        rs16.decode_device(k, m, SB, d_x.ptr, d_f.ptr + oo, d_r.ptr, d_f.ptr + ro, 0, m, engine=eng, check=True)
    assert e.value.kind == "InvalidArgument"
    # consistent dressed flags pass the check and restore
    rm[:] = True
    buf, oo, ro = flag_buffer(dress(np.zeros(k, bool), 0), dress(rm, 5, value), 0)
    d_f.upload(buf)
    rs16.decode_device(k, m, SB, d_x.ptr, d_f.ptr + oo, d_r.ptr, d_f.ptr + ro, 0, m, engine=eng, check=True)
    same(d_x.download(shape=(k, SB)), original, "originals")


# ---------------------------------------------------------------------------
# Device shard arrays start on a 64-byte boundary (include/rs16.h)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [8, 16, 32])
def test_misaligned_shard_arrays_are_refused(eng, delta):
    # every wrapper that takes a caller's device shard array: InvalidArgument
    # for a base at +8 / +16 / +32, and no byte of the memory around and
    # inside the arrays changes (nothing was launched); the same arguments on
    # 64-byte boundaries are accepted
    k = m = 4
    n = 2  # stripes
    size = 8192
    guard = (np.arange(size) * 37 % 251).astype(np.uint8)
    d = DeviceArray.from_numpy(eng, guard)
    assert d.ptr % 64 == 0
    a0, b0 = d.ptr + 1024, d.ptr + 4096  # 2 KiB and more each
    fl = DeviceArray.from_numpy(eng, np.array([0, 0x80, 0xFF, 2, 0x40, 0, 0, 0] * 2, np.uint8))
    fo, fr = fl.ptr, fl.ptr + 4  # originals 0,1,1,1 / recovery 1,0,0,0 (dressed), twice for two stripes
    plan = rs16.UpdatePlan(k, m, [1, 2], engine=eng)
    calls = {
        "encode": lambda a, b: rs16.encode_device(k, m, SB, a, b, engine=eng),
        "encode_batch": lambda a, b: rs16.encode_device_batch(k, m, SB, n, a, k * SB, b, m * SB, engine=eng),
        "decode": lambda a, b: rs16.decode_device(k, m, SB, a, fo, b, fr, 3, 1, engine=eng),
        "decode_nothing": lambda a, b: rs16.decode_device(k, m, SB, a, fo, b, fr, 4, 0, engine=eng),
        "decode_batch": lambda a, b: rs16.decode_device_batch(k, m, SB, n, a, k * SB, fo, b, m * SB, fr, 3, 1,
                                                              engine=eng),
        "decode_varied": lambda a, b: rs16.decode_device_batch_varied(k, m, SB, n, a, k * SB, fo, 8, b, m * SB, fr,
                                                                      8, [3, 3], [1, 1], engine=eng),
        "update": lambda a, b: plan.apply(SB, a, b),
        "xor": lambda a, b: eng.xor(a, b, 4 * SB),
    }
    one = {
        "mul": lambda a: eng.mul(a, 4 * SB, 1234),
        "fft": lambda a: eng.fft(a, 8, SB, 0, 8, 8, 8),
        "ifft": lambda a: eng.ifft(a, 8, SB, 0, 8, 8, 8),
        "fft_skew_end": lambda a: eng.fft_skew_end(a, 8, SB, 0, 8, 8),
        "ifft_skew_end": lambda a: eng.ifft_skew_end(a, 8, SB, 0, 8, 8),
        "xor_within": lambda a: eng.xor_within(a, 8, SB, 0, 4, 4),
        "formal_derivative": lambda a: eng.formal_derivative(a, 8, SB),
    }

    def refused(f, *args):
        with pytest.raises(rs16.Error) as e:
            f(*args)
        assert e.value.kind == "InvalidArgument", e.value

    try:
        for name, f in calls.items():
            refused(f, a0 + delta, b0)
            refused(f, a0, b0 + delta)
            refused(f, a0 + delta, b0 + delta)
        for name, f in one.items():
            refused(f, a0 + delta)
        # a preparation is not consumed by a refused call
        rs16.decode_prepare(k, m, SB, fo, fr, 3, 1, engine=eng)
        prepared = lambda a, b: rs16.decode_device_prepared(k, m, SB, a, b, engine=eng)  # noqa: E731
        refused(prepared, a0 + delta, b0)
        refused(prepared, a0, b0 + delta)
        eng.synchronize()
        assert np.array_equal(d.download(), guard), "a refused call wrote device memory"
        prepared(a0, b0)
        for f in calls.values():
            f(a0, b0)
        for f in one.values():
            f(a0)
        eng.synchronize()
    finally:
        eng.synchronize()
        plan.close()


@pytest.mark.parametrize("k,m,diag", [(100, 100, 0), (300, 300, NC)], ids=["column-100", "pass-300"])
def test_base_64_mod_128(eng, k, m, diag):
    # originals and recovery at a base = 64 (mod 128): the smallest alignment
    # the contract allows.  Encode against the oracle, decode back.
    original = generate_original(k, SB, 77)
    want = O.encode(k, m, original)
    om, rm = make_masks(k, m, "half", 3)
    g = np.full(64, 0x6B, np.uint8)
    d_o = DeviceArray.from_numpy(eng, np.concatenate([g, original.reshape(-1), g]))
    d_r = DeviceArray.from_numpy(eng, np.full(m * SB + 128, 0x6B, np.uint8))
    assert d_o.ptr % 128 == 0 and d_r.ptr % 128 == 0
    po, pr = d_o.ptr + 64, d_r.ptr + 64
    buf, oo, ro = flag_buffer(dress(om, 4), dress(rm, 0), 3)
    d_f = DeviceArray.from_numpy(eng, buf)
    old = eng.set_diagnostics(diag)
    try:
        rs16.encode_device(k, m, SB, po, pr, engine=eng)
        got = d_r.download()
        assert (got[:64] == 0x6B).all() and (got[-64:] == 0x6B).all()
        same(got[64:-64].reshape(m, SB), want, "recovery")
        rec = given(want, rm)
        d_r.upload(np.concatenate([g, rec.reshape(-1), g]))
        d_o.upload(np.concatenate([g, holes(original, om).reshape(-1), g]))
        rs16.decode_device(k, m, SB, po, d_f.ptr + oo, pr, d_f.ptr + ro, int(om.sum()), int(rm.sum()), engine=eng,
                           check=True)
    finally:
        eng.set_diagnostics(old)
    got = d_o.download()
    assert (got[:64] == 0x6B).all() and (got[-64:] == 0x6B).all()
    same(got[64:-64].reshape(k, SB), original, "originals")
    assert np.array_equal(d_r.download()[64:-64].reshape(m, SB), rec)
