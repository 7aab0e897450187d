"""Every slot of launch_pass's kernel lookup, through a launch of its own.

The pass kernels are instantiated in two translation units and found through
a (program, tile bits T, narrow variant) lookup (rs16_pass_common.hpp
PassKernel, rs16_pass_launch.hip): a wrong kernel in a slot shows only in a
launch through that slot.  So this runs, at 64-byte shards and byte for byte
against the oracle (src/rate/rate_high.rs:44-83, 168-247; the Engine ops
src/engine.rs:150-195 with NoSimd as the bit-exact target):

  * with RS16_DIAG_NO_COLUMN (every size through the pass codec), k = m = 2^j
    for j = 0 .. 15: the encode; the decode of every original lost as shipped
    (identity multipliers: the ENC_* programs as decode passes) and with
    RS16_DIAG_NO_IDENTITY (DEC_FIRST, ENC_MID, DEC_HALF_LAST, or
    DEC_HALF_SINGLE); the decode of about half of the originals lost at seeded
    random positions with as many random recovery shards (DEC_SINGLE up to 256
    work rows, else DEC_FIRST, DEC_MID, DEC_LAST), from j = 8 on also without
    the two small kernels;
  * one decode of 1 % contiguous loss at j = 15 as shipped (mid_direct_kernel
    and tile_last_kernel);
  * Engine fft / ifft over 2^L rows, L = 0 .. 16 (GEN_FFT / GEN_IFFT at every
    one-pass T and every split into a strided and a contiguous pass);
  * ENC_MID's narrow variants: a 2^14-row stripe (variant 1) and a 2^15-row
    stripe (variant 2 in the encode, 3 in the identity decode), each also with
    RS16_DIAG_WIDE_TWIDDLES (the 12-lookup kernel of the same slot).
"""
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu
SB = 64
PASSES = rs16.DIAG_NO_COLUMN
NO_SMALL = rs16.DIAG_NO_MID_DIRECT | rs16.DIAG_NO_TILE_LAST


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(j):
    """Originals and the oracle's recovery shards of k = m = 2^j (computed once, read-only)."""
    k = 1 << j
    original = generate_original(k, SB, 100 + j)
    recovery = O.encode(k, k, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def masks(j, loss):
    """(received originals, received recovery) of a loss pattern."""
    k = 1 << j
    om, rm = np.ones(k, bool), np.zeros(k, bool)
    if loss == "all":  # every original lost, every recovery shard given
        om[:] = False
        rm[:] = True
    elif loss == "half":  # about half lost at random positions, as many random recovery shards
        rng = np.random.default_rng(1000 + j)
        n = max(1, k // 2)
        om[rng.permutation(k)[:n]] = False
        rm[rng.permutation(k)[:n]] = True
    else:  # 1 %: the last originals lost, the first recovery shards given
        n = max(1, k // 100)
        om[k - n:] = False
        rm[:n] = True
    return om, rm


@functools.lru_cache(maxsize=None)
def oracle_decode(j, loss):
    original, recovery = stripe(j)
    om, rm = masks(j, loss)
    dec = O.Decoder("default", "nosimd", 1 << j, 1 << j, SB)
    for i in np.flatnonzero(om):
        dec.add_original_shard(int(i), original[i])
    for i in np.flatnonzero(rm):
        dec.add_recovery_shard(int(i), recovery[i])
    want = original.copy()
    for i, shard in dec.decode().items():
        want[i] = shard
    assert np.array_equal(want, original)  # (the oracle restores what was lost)
    want.setflags(write=False)
    return want


def encode(eng, j, diag):
    k = 1 << j
    original, recovery = stripe(j)
    d_o = DeviceArray.from_numpy(eng, original)
    d_r = DeviceArray.from_numpy(eng, np.full((k, SB), 0x5A, np.uint8))
    old = eng.set_diagnostics(diag)
    try:
        rs16.encode_device(k, k, SB, d_o.ptr, d_r.ptr, engine=eng)
    finally:
        eng.set_diagnostics(old)
    assert np.array_equal(d_r.download(shape=(k, SB)), recovery)


def decode(eng, j, loss, diag):
    k = 1 << j
    original, recovery = stripe(j)
    om, rm = masks(j, loss)
    want = oracle_decode(j, loss)
    holes = original.copy()
    holes[~om] = 0xA5  # lost rows hold garbage
    d_x = DeviceArray.from_numpy(eng, holes)
    d_r = DeviceArray.from_numpy(eng, recovery)
    d_of = DeviceArray.from_numpy(eng, om.astype(np.uint8))
    d_rf = DeviceArray.from_numpy(eng, rm.astype(np.uint8))
    old = eng.set_diagnostics(diag)
    try:
        rs16.decode_device(k, k, SB, d_x.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, int(om.sum()), int(rm.sum()), engine=eng,
                           check=True)
    finally:
        eng.set_diagnostics(old)
    assert np.array_equal(d_x.download(shape=(k, SB)), want)


J = list(range(16))


@pytest.mark.parametrize("j", J)
def test_encode(eng, j):
    encode(eng, j, PASSES)


@pytest.mark.parametrize("j", J)
def test_decode_all_lost_identity(eng, j):
    decode(eng, j, "all", PASSES)


@pytest.mark.parametrize("j", J)
def test_decode_all_lost_evaluated(eng, j):
    decode(eng, j, "all", PASSES | rs16.DIAG_NO_IDENTITY)


@pytest.mark.parametrize("j", J)
def test_decode_half_lost(eng, j):
    decode(eng, j, "half", PASSES)
    if j >= 8:
        decode(eng, j, "half", PASSES | NO_SMALL)


def test_decode_one_percent_contiguous_as_shipped(eng):
    decode(eng, 15, "1%", 0)


@pytest.mark.parametrize("j", [14, 15])
@pytest.mark.parametrize("wide", [0, rs16.DIAG_WIDE_TWIDDLES], ids=["narrow", "wide"])
def test_enc_mid_narrow_variants(eng, j, wide):
    encode(eng, j, PASSES | wide)
    decode(eng, j, "all", PASSES | wide)


@pytest.mark.parametrize("L", list(range(17)))
def test_engine_fft_ifft(eng, L):
    n = 1 << L
    x = np.random.default_rng(L).integers(0, 256, (n, SB), dtype=np.uint8)
    d = DeviceArray.from_numpy(eng, x)
    old = eng.set_diagnostics(PASSES)
    try:
        eng.fft(d.ptr, n, SB, 0, n, n, 0)
        got_fft = d.download(shape=x.shape)
        d.upload(x)
        eng.ifft(d.ptr, n, SB, 0, n, n, 0)
        got_ifft = d.download(shape=x.shape)
    finally:
        eng.set_diagnostics(old)
    want = x.copy()
    O.fft(want, 0, n, n, 0)
    assert np.array_equal(got_fft, want)
    want = x.copy()
    O.ifft(want, 0, n, n, 0)
    assert np.array_equal(got_ifft, want)
