"""Row addressing of the pass kernels: the full-item fast path (one base
address per wave and array, launch-constant row strides, PassArgs::rs_in) and
the general path (per-row limits, zero page, partial slabs, 64-bit lane
offsets) must give the same bytes.  Every case is bit-exact against the
oracle, at the smallest shapes that reach the pass kernels (stripes above
2048 rows) with both paths in one launch: tiles that straddle the row limit,
shard widths with 1 slab, a slab count that is no power of two and a partial
last slab, forced 64-bit lane offsets, batched stripes and a row stride wider
than the slice."""
import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

gpu = pytest.mark.gpu

# 64 B: one (partial) slab; 192 B: 24 quads; 1024 B: 128 quads, full slabs at
# every Q; 1088 B: 136 quads, 3 / 5 / 9 slabs with a partial last one
SHARD_BYTES = (64, 192, 1024, 1088)

_cache = {}


def _stripe(k, m, sb):
    """(originals, the oracle's recovery) of a k:m x sb stripe, computed once."""
    key = (k, m, sb)
    if key not in _cache:
        orig = generate_original(k, sb, k + m + sb)
        rec = O.encode(k, m, orig)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (orig, rec)
    return _cache[key]


def _encode(eng, k, m, sb):
    orig, want = _stripe(k, m, sb)
    d_o = DeviceArray.from_numpy(eng, orig)
    d_r = DeviceArray.from_numpy(eng, np.full(m * sb, 0x77, np.uint8))
    rs16.encode_device(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_r.download(shape=(m, sb)), want)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)  # the originals stay


def _decode(eng, k, m, sb, lost):
    """Decode with the originals `lost` (bool mask) lost and as many recovery
    shards received, chosen at random; garbage in the lost slots."""
    orig, rec = _stripe(k, m, sb)
    nlost = int(lost.sum())
    rm = np.zeros(m, bool)
    rm[np.random.default_rng(k + nlost).choice(m, nlost, replace=False)] = True
    held = orig.copy()
    held[lost] = 0xA5
    got_r = rec.copy()
    got_r[~rm] = 0x5A
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, got_r)
    d_of = DeviceArray.from_numpy(eng, (~lost).astype(np.uint8))
    d_rf = DeviceArray.from_numpy(eng, rm.astype(np.uint8))
    rs16.decode_device(k, m, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, k - nlost, nlost, engine=eng, check=True)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)
    assert np.array_equal(d_r.download(shape=(m, sb)), got_r)  # the recovery stays


@gpu
@pytest.mark.parametrize("sb", SHARD_BYTES)
@pytest.mark.parametrize("k,m", [(3000, 2500), (2049, 2049)])
def test_encode_full_and_partial_tiles(k, m, sb):
    # first pass: tiles below, across and above row k; last pass: the same at row m
    _encode(rs16.default_engine(), k, m, sb)


@gpu
@pytest.mark.parametrize("sb", SHARD_BYTES)
@pytest.mark.parametrize("k", [2048, 4096])
def test_identity_decode(k, sb):
    # every original lost, recovery 0 .. k received: the encoder's kernels as the decode's passes
    eng = rs16.default_engine()
    orig, rec = _stripe(k, k, sb)
    d_o = DeviceArray.from_numpy(eng, np.full(k * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(k, np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, k, engine=eng, check=True)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)
    assert np.array_equal(d_r.download(shape=(k, sb)), rec)


@gpu
@pytest.mark.parametrize("sb", SHARD_BYTES)
def test_general_decode_random_losses(sb):
    k = m = 3000
    lost = np.zeros(k, bool)
    lost[np.random.default_rng(sb).choice(k, 1100, replace=False)] = True
    _decode(rs16.default_engine(), k, m, sb, lost)


@gpu
def test_forced_64bit_lane_offsets():
    # (no fast path in such a launch: PassArgs::full_lanes needs 32-bit lane offsets)
    old = rs16.set_diagnostics(rs16.DIAG_FORCE_VOFF64)
    try:
        eng = rs16.default_engine()
        _encode(eng, 3000, 2500, 192)
        _decode(eng, 4096, 4096, 1024, np.ones(4096, bool))
    finally:
        rs16.set_diagnostics(old)


@gpu
@pytest.mark.parametrize("k,m,sb", [(4096, 4096, 128), (3000, 2500, 1088)])
def test_batched_stripes(k, m, sb):
    # 3 stripes in one launch: the workgroup index splits into (stripe, tile
    # of the stripe) by the launch's tiles per stripe; encode ...
    eng = rs16.default_engine()
    n, pad = 3, 64
    so, sr = k * sb + pad, m * sb + pad
    stripes = [generate_original(k, sb, 7 * i + k) for i in range(n)]
    recs = [O.encode(k, m, o) for o in stripes]
    host_o = np.full(n * so, 0xEE, np.uint8)
    for i, o in enumerate(stripes):
        host_o[i * so:i * so + k * sb] = o.reshape(-1)
    d_o = DeviceArray.from_numpy(eng, host_o)
    d_r = DeviceArray.from_numpy(eng, np.full(n * sr, 0x77, np.uint8))
    rs16.encode_device_batch(k, m, sb, n, d_o.ptr, so, d_r.ptr, sr, engine=eng)
    got = d_r.download(shape=(n * sr,))
    for i in range(n):
        assert np.array_equal(got[i * sr:i * sr + m * sb].reshape(m, sb), recs[i]), i
        assert (got[i * sr + m * sb:(i + 1) * sr] == 0x77).all(), i
    # ... and back: the first min(k, m) originals lost in every stripe
    nl = min(k, m)
    om = np.ones(k, np.uint8)
    om[:nl] = 0
    rm = np.zeros(m, np.uint8)
    rm[:nl] = 1
    for i in range(n):
        host_o[i * so:i * so + nl * sb] = 0xA5
    d_o.upload(host_o)
    d_of, d_rf = DeviceArray.from_numpy(eng, om), DeviceArray.from_numpy(eng, rm)
    rs16.decode_device_batch(k, m, sb, n, d_o.ptr, so, d_of.ptr, d_r.ptr, sr, d_rf.ptr, k - nl, nl, engine=eng)
    back = d_o.download(shape=(n * so,))
    for i in range(n):
        assert np.array_equal(back[i * so:i * so + k * sb].reshape(k, sb), stripes[i]), i
        assert (back[i * so + k * sb:(i + 1) * so] == 0xEE).all(), i


@gpu
@pytest.mark.parametrize("slices", [2, 3])
def test_row_stride_wider_than_the_slice(slices):
    # column slices: the passes work on a slice of the caller's rows, whose
    # stride (the shard) is not the slice's width
    eng = rs16.default_engine()
    eng.set_slices(slices)
    try:
        _encode(eng, 3000, 2500, 1024)
        _decode(eng, 4096, 4096, 1024, np.ones(4096, bool))
    finally:
        eng.set_slices(1)


def test_division_constants():
    # fast_div (rs16_internal.hpp) against n / d on the host: every divisor up
    # to 8192 (slabs per row of shards up to 1 MiB, tiles per stripe of up to
    # 65536 rows) and divisors around the powers of two up to 2^32, each over
    # the low and the high end of the 32-bit range and a stride through all of it
    from rs16._lib import lib
    check = lib().rs16_host_fast_div_check
    divisors = set(range(1, 8193))
    for s in range(13, 32):
        divisors.update(((1 << s) - 1, 1 << s, (1 << s) + 1, 3 << (s - 2)))
    divisors.update((0xFFFFFFFF, 0xFFFFFFFE, 0x80000001, 641, 6700417, 65521 * 65537))
    for d in sorted(divisors):
        assert check(d, 0, 20000, 1) == 0, d
        assert check(d, 2 ** 32 - 20000, 20000, 1) == 0, d
        assert check(d, d - 1, 20000, 214013) == 0, d
        # around the multiples of d: q d - 1 and q d for the largest q
        top = (2 ** 32 - 1) // d * d
        assert check(d, top - 1, 2, 1) == 0, d
        if d > 1:
            assert check(d, d - 1, 20000, d) == 0 and check(d, d, 20000, d) == 0, d
