"""Wave-private table staging of the encoder-family passes at T >= 7
(rs16_pass.hpp WaveStaged): every wave stages the tables of its first layer
block itself and starts its butterflies without a workgroup barrier; the
tables of the later blocks are committed without a barrier of their own.
Every case is bit-exact against the oracle, at the smallest stripes whose
passes are those kernels: 2^15 rows (tile bits T = 7 / 8 / 7) and 2^14 rows
(T = 7 throughout), at shard widths of one partial slab (64 and 192 B: 8 and
24 quads), of several slabs with a partial last one (1088 B: 136 quads; no
launch of these three widths has the full-item stores, PassArgs::full_lanes)
and of full slabs only (512 B: 64 quads, the benchmark's kind of launch),
zero-gathered rows and a partial last recovery tile,
the identity decode (the same kernels as the decode's passes, with and
without the received counts), two batched stripes, and the general addressing
paths (wide twiddles, forced 64-bit lane offsets)."""
import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

gpu = pytest.mark.gpu

SHARD_BYTES = (64, 192, 1088)

_cache = {}


def _stripe(k, m, sb, seed=0):
    """(originals, the oracle's recovery) of a k:m x sb stripe, computed once."""
    key = (k, m, sb, seed)
    if key not in _cache:
        orig = generate_original(k, sb, k + m + sb + seed)
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


def _identity_decode(eng, k, sb, check):
    # every original lost, recovery 0 .. k received: the encoder's kernels as
    # the decode's passes; check=True has the first and last pass count the
    # received flags (PassArgs::rcount)
    orig, rec = _stripe(k, k, sb)
    d_o = DeviceArray.from_numpy(eng, np.full(k * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(k, np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, k, engine=eng, check=check)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)
    assert np.array_equal(d_r.download(shape=(k, sb)), rec)  # the recovery stays


@gpu
@pytest.mark.parametrize("sb", SHARD_BYTES)
@pytest.mark.parametrize("n", [16384, 32768])
def test_encode(n, sb):
    _encode(rs16.default_engine(), n, n, sb)


@gpu
@pytest.mark.parametrize("n", [16384, 32768])
def test_full_item_launch(n):
    # 512-byte shards: every lane of every item holds a quad (one slab at
    # T = 7, two at T = 8), the launches of the benchmark's kind; encode, and
    # the identity decode at 16384
    eng = rs16.default_engine()
    _encode(eng, n, n, 512)
    if n == 16384:
        _identity_decode(eng, n, 512, True)


@gpu
@pytest.mark.parametrize("k,m", [(20000, 20000), (32768, 20000)])
def test_encode_zero_rows_and_partial_last_tile(k, m):
    # first pass: tiles below, across and above row k (zero-gathered rows);
    # last pass: a partial last recovery tile (20000 = 156 x 128 + 32)
    _encode(rs16.default_engine(), k, m, 192)


@gpu
@pytest.mark.parametrize("k,check", [(16384, False), (32768, True)])
def test_identity_decode(k, check):
    _identity_decode(rs16.default_engine(), k, 192, check)


@gpu
def test_two_batched_stripes():
    eng = rs16.default_engine()
    k = m = 16384
    sb, n, pad = 64, 2, 64
    so, sr = k * sb + pad, m * sb + pad
    pairs = [_stripe(k, m, sb), _stripe(k, m, sb, seed=1)]
    host_o = np.full(n * so, 0xEE, np.uint8)
    for i, (o, _) in enumerate(pairs):
        host_o[i * so:i * so + k * sb] = o.reshape(-1)
    d_o = DeviceArray.from_numpy(eng, host_o)
    d_r = DeviceArray.from_numpy(eng, np.full(n * sr, 0x77, np.uint8))
    rs16.encode_device_batch(k, m, sb, n, d_o.ptr, so, d_r.ptr, sr, engine=eng)
    got = d_r.download(shape=(n * sr,))
    for i, (_, rec) in enumerate(pairs):
        assert np.array_equal(got[i * sr:i * sr + m * sb].reshape(m, sb), rec), i
        assert (got[i * sr + m * sb:(i + 1) * sr] == 0x77).all(), i
    # ... and back: every original lost in both stripes
    for i in range(n):
        host_o[i * so:i * so + k * sb] = 0xA5
    d_o.upload(host_o)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    rs16.decode_device_batch(k, m, sb, n, d_o.ptr, so, d_of.ptr, d_r.ptr, sr, d_rf.ptr, 0, k, engine=eng)
    back = d_o.download(shape=(n * so,))
    for i, (o, _) in enumerate(pairs):
        assert np.array_equal(back[i * so:i * so + k * sb].reshape(k, sb), o), i
        assert (back[i * so + k * sb:(i + 1) * so] == 0xEE).all(), i


@gpu
def test_wide_twiddles():
    # the 12-lookup middle pass (no narrow variant) through the new staging
    old = rs16.set_diagnostics(rs16.DIAG_WIDE_TWIDDLES)
    try:
        eng = rs16.default_engine()
        _encode(eng, 32768, 32768, 192)
        _identity_decode(eng, 16384, 192, False)
    finally:
        rs16.set_diagnostics(old)


@gpu
def test_forced_64bit_lane_offsets():
    # (no full-item fast path in such a launch: the general row addressing)
    old = rs16.set_diagnostics(rs16.DIAG_FORCE_VOFF64)
    try:
        eng = rs16.default_engine()
        _encode(eng, 16384, 16384, 1088)
        _identity_decode(eng, 32768, 192, True)
    finally:
        rs16.set_diagnostics(old)
