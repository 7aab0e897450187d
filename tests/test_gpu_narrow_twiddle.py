"""The narrow-twiddle variants of the middle passes (rs16_pass.hpp NarrowVar;
launch_pass picks one per launch from first_narrow_layer) against the
12-lookup multiply everywhere (RS16_DIAG_WIDE_TWIDDLES) and the oracle.

Every case runs twice, default and wide; both results must equal each other
and the oracle's (src/rate/rate_high.rs:44-83, 168-247; rate_low.rs alike),
byte for byte.  The row counts select the launches: 2^15-row stripes have
one wide layer next to narrow ones in the middle pass (encode: the IFFT's,
identity decode: the FFT's), the 65536-row general decode and the stripes of
up to 4096 rows are narrow in every layer, and 60000:3000 / 3000:60000 run
at skews that are neither 0 nor the stripe's size.  Shard widths 64 B and
192 B: one full and one partial slab of the smallest rows the kernels take.
"""
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu
WIDE = rs16.DIAG_WIDE_TWIDDLES


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, sb):
    """Originals and the oracle's recovery shards (computed once, read-only)."""
    original = generate_original(k, sb, k + m + sb)
    recovery = O.encode(k, m, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def masks(k, m, loss):
    """(received originals, received recovery) of a loss pattern."""
    rng = np.random.default_rng(k * 3 + m)
    om, rm = np.ones(k, bool), np.zeros(m, bool)
    if loss == "all":  # every original lost (at most m of them), recovery 0.. given
        n = min(k, m)
        om[:n] = False
        rm[:n] = True
    else:  # `loss` originals lost, scattered; as many scattered recovery shards given
        om[rng.permutation(k)[:loss]] = False
        rm[rng.permutation(m)[:loss]] = True
    return om, rm


def oracle_decode(original, recovery, om, rm):
    k, sb = original.shape
    dec = O.Decoder("default", "nosimd", k, recovery.shape[0], sb)
    for i in np.flatnonzero(om):
        dec.add_original_shard(int(i), original[i])
    for i in np.flatnonzero(rm):
        dec.add_recovery_shard(int(i), recovery[i])
    want = original.copy()
    for i, shard in dec.decode().items():
        want[i] = shard
    return want


def run_both(eng, diag, fn):
    """fn() under `diag` and under `diag | WIDE`."""
    out = []
    for d in (diag, diag | WIDE):
        old = eng.set_diagnostics(d)
        try:
            out.append(fn())
        finally:
            eng.set_diagnostics(old)
    return out


def check_encode(eng, k, m, sb, diag):
    original, recovery = stripe(k, m, sb)
    d_o = DeviceArray.from_numpy(eng, original)

    def enc():
        d_r = DeviceArray.from_numpy(eng, np.full((m, sb), 0x5A, np.uint8))
        rs16.encode_device(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
        return d_r.download(shape=(m, sb))

    narrow, wide = run_both(eng, diag, enc)
    assert np.array_equal(narrow, wide)
    assert np.array_equal(narrow, recovery)


def check_decode(eng, k, m, sb, diag, loss):
    original, recovery = stripe(k, m, sb)
    om, rm = masks(k, m, loss)
    want = oracle_decode(original, recovery, om, rm)
    assert np.array_equal(want, original)  # (the oracle restores what was lost)
    d_r = DeviceArray.from_numpy(eng, recovery)
    d_of = DeviceArray.from_numpy(eng, om.astype(np.uint8))
    d_rf = DeviceArray.from_numpy(eng, rm.astype(np.uint8))
    holes = original.copy()
    holes[~om] = 0xA5  # lost rows hold garbage

    def dec():
        d_x = DeviceArray.from_numpy(eng, holes)
        rs16.decode_device(k, m, sb, d_x.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, int(om.sum()), int(rm.sum()), engine=eng,
                           check=True)
        return d_x.download(shape=(k, sb))

    narrow, wide = run_both(eng, diag, dec)
    assert np.array_equal(narrow, wide)
    assert np.array_equal(narrow, want)


SB = [64, 192]


@pytest.mark.parametrize("sb", SB)
def test_encode_32768(eng, sb):
    # the IFFT's wide layer 0 (skew 2^15) next to 15 narrow layers in one launch
    check_encode(eng, 32768, 32768, sb, 0)


@pytest.mark.parametrize("diag", [0, rs16.DIAG_NO_IDENTITY], ids=["identity", "evaluated"])
@pytest.mark.parametrize("sb", SB)
def test_decode_32768_all_lost(eng, sb, diag):
    # the half decode's middle pass: the FFT's layer 0 is the wide one
    check_decode(eng, 32768, 32768, sb, diag, "all")


@pytest.mark.parametrize("sb", SB)
def test_decode_30000_all_lost(eng, sb):
    check_decode(eng, 30000, 30000, sb, 0, "all")


@pytest.mark.parametrize("sb", SB)
def test_decode_32768_one_percent_scattered(eng, sb):
    # general decode: DEC_MID over 65536 rows, narrow in every layer
    check_decode(eng, 32768, 32768, sb, 0, 328)


@pytest.mark.parametrize("k", [2048, 4096])
@pytest.mark.parametrize("sb", SB)
def test_round_trip_small_stripes_through_the_passes(eng, sb, k):
    # every layer of every direction is narrow
    check_encode(eng, k, k, sb, rs16.DIAG_NO_COLUMN)
    check_decode(eng, k, k, sb, rs16.DIAG_NO_COLUMN, "all")
    check_decode(eng, k, k, sb, rs16.DIAG_NO_COLUMN | rs16.DIAG_NO_IDENTITY, "all")
    check_decode(eng, k, k, sb, rs16.DIAG_NO_COLUMN, k // 50)


@pytest.mark.parametrize("k,m", [(60000, 3000), (3000, 60000)])
@pytest.mark.parametrize("sb", SB)
def test_round_trip_uneven_rates(eng, sb, k, m):
    # skews that are neither 0 nor a power of two: the host's choice against
    # the largest indices the launches really form
    check_encode(eng, k, m, sb, 0)
    check_decode(eng, k, m, sb, 0, "all" if k < m else 3000)
