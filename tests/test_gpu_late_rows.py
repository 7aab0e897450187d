"""Late row requests of the wave-staged passes (rs16_pass.hpp LateRows,
pass_kernel_late): a launch none of whose waves needs the general row loads
requests D row pairs ahead of the table commit and the rest from inside the
first layer.  launch_pass decides per launch (PassConsts::late_rows): 32-bit
lane offsets, no row mask, no RS16_DIAG_NO_LATE_ROWS, and -- the gathering
first pass -- a row limit a_count that cuts through no wave's rows.

Every GPU case is bit-exact against the oracle at the smallest stripes whose
passes are these kernels (2^14 rows: T = 7 throughout; 2^15 rows: T = 7 / 8 /
7), and asserts through the host hook (rs16_host_pass_consts_rows, the
function launch_pass calls) which of its launches take the variant.  The
launches of a stripe are written out below as the engine plans them
(rs16_engine.cpp encode_high_fused / decode_passes: a chunk of 2^L rows in
passes of L / 2 contiguous, L - L / 2 strided and L / 2 contiguous row bits).

The row limit 20000 (20000:20000 x 192 B) does not cut a wave: the first pass
of a 2^15-row chunk is T = 7 at lo = 0, whose waves hold 16 consecutive rows,
and 20000 = 1250 x 16 -- it cuts a tile (20000 = 156 x 128 + 32), and the
waves of that tile lie wholly below or wholly above it.  That launch takes
the variant (asserted, with the integer model's word for it); the case of a
limit inside a wave is 19992:20000 (19992 = 1249 x 16 + 8), which must not.

The CPU case compares the hook's decision for the gathering pass with an
integer model of "some wave's row range contains a_count strictly inside",
written out from WaveRows' definition, over T in {7, 8}, lo in 0 .. 8."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import PassConsts, lib
from rs16.device import DeviceArray
from rs16.util import generate_original

gpu = pytest.mark.gpu

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


# ---------------------------------------------------------------------------
# The launches of a stripe and the hook's word on each.
# ---------------------------------------------------------------------------
def _prog(name):
    n = lib().rs16_prog_count()
    return {lib().rs16_prog_name(i).decode(): i for i in range(n)}[name]


def _late(prog, T, lo, sb, a_count, diag, chunk=0, row_base_in=0):
    out = PassConsts()
    assert lib().rs16_host_pass_consts_rows(_prog(prog), T, lo, sb, sb, sb, sb, sb // 8, chunk, row_base_in, 0, a_count,
                                            diag, C.byref(out))
    return out.late_rows


def _launches(rows, a_count):
    """(prog, T, lo, a_count) of the three passes over a chunk of `rows` (a power of two) rows."""
    L = rows.bit_length() - 1
    lo, hi = L // 2, L - L // 2
    return [("ENC_FIRST", lo, 0, a_count), ("ENC_MID", hi, lo, 0), ("ENC_LAST", lo, 0, 0)]


def _encode_late(k, m, sb, diag=0):
    chunk = 1 << (m - 1).bit_length()
    return [_late(p, T, lo, sb, k if p == "ENC_FIRST" else 0, diag) for p, T, lo, _ in _launches(chunk, k)]


def _decode_late(k, sb, diag=0):
    # the identity decode of k:k: the received half (k rows) through the
    # encoder's passes; the decode's segment boundary and first gather row
    # (multiples of every pass's tile span) travel with the launch
    return [max(_late(p, T, lo, sb, k if p == "ENC_FIRST" else 0, diag, chunk=k, row_base_in=base)
                for base in (0, k)) for p, T, lo, _ in _launches(k, k)]


# ---------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sb", [512, 64, 1088])
@pytest.mark.parametrize("n", [16384, 32768])
def test_encode(n, sb):
    # full slabs (512 B), one partial slab (64 B), slabs with a partial last
    # one (1088 B): every launch takes the variant
    assert _encode_late(n, n, sb) == [1, 1, 1]
    _encode(rs16.default_engine(), n, n, sb)


@gpu
def test_encode_zero_page_waves():
    # the row limit 24576 = 192 x 128 is aligned: the waves of the tiles above
    # it read the zero page inside the variant
    assert _encode_late(24576, 32768, 192) == [1, 1, 1]
    _encode(rs16.default_engine(), 24576, 32768, 192)


@gpu
def test_encode_limit_inside_a_tile():
    # 20000 = 156 x 128 + 32 = 1250 x 16: the limit cuts a tile between two of
    # its waves (16 consecutive rows each), none of which needs the general
    # loads -- the variant, with direct and zero-page waves in one workgroup
    assert _wave_cut(7, 0, 20000) is False
    assert _encode_late(20000, 20000, 192) == [1, 1, 1]
    _encode(rs16.default_engine(), 20000, 20000, 192)


@gpu
def test_encode_limit_inside_a_wave():
    # 19992 = 1249 x 16 + 8: the limit cuts a wave, the first pass keeps
    # pass_kernel (its general row loads); the other two passes do not gather
    assert rs16.use_high_rate(19992, 20000)  # (the fused three-pass encoder)
    assert _wave_cut(7, 0, 19992) is True
    assert _encode_late(19992, 20000, 192) == [0, 1, 1]
    _encode(rs16.default_engine(), 19992, 20000, 192)


@gpu
@pytest.mark.parametrize("check", [False, True], ids=["plain", "check"])
@pytest.mark.parametrize("k", [16384, 32768])
def test_identity_decode(k, check):
    assert _decode_late(k, 192) == [1, 1, 1]
    _identity_decode(rs16.default_engine(), k, 192, check)


@gpu
def test_two_batched_stripes():
    eng = rs16.default_engine()
    k = m = 16384
    sb, n, pad = 64, 2, 64
    assert _encode_late(k, m, sb) == [1, 1, 1]  # (per stripe: one geometry)
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
    assert np.array_equal(d_o.download(shape=(n * so,)), host_o)  # originals and their padding stay


@gpu
@pytest.mark.parametrize("diag,late", [("DIAG_NO_LATE_ROWS", 0), ("DIAG_FORCE_VOFF64", 0), ("DIAG_WIDE_TWIDDLES", 1)])
def test_diagnostics(diag, late):
    flag = getattr(rs16, diag)
    assert _encode_late(32768, 32768, 192, flag) == [late] * 3
    assert _decode_late(16384, 192, flag) == [late] * 3
    old = rs16.set_diagnostics(flag)
    try:
        eng = rs16.default_engine()
        _encode(eng, 32768, 32768, 192)
        _identity_decode(eng, 16384, 192, True)
    finally:
        rs16.set_diagnostics(old)


# ---------------------------------------------------------------------------
# CPU: the launch rule of the gathering pass against an integer model.
# ---------------------------------------------------------------------------
R = 4                    # row bits a lane holds in registers (Geo<T>::R at T >= 6)
HWS = {7: 1, 8: 2}       # row sets per wave (Geo<T>::HWS: 64 / 32 quads per tile row)
B_HIGH = 3               # tiles b_high = 0 .. 2 of every b_low


def _wave_bases(T, lo, n_high=B_HIGH):
    """WaveRows<T, layout A>::base of every wave of the tiles (b_low, b_high < n_high)."""
    b_low = np.arange(1 << lo, dtype=np.int64)[:, None, None]
    b_high = np.arange(n_high, dtype=np.int64)[None, :, None]
    w = np.arange((1 << (T - R)) // HWS[T], dtype=np.int64)[None, None, :]
    return (b_low + (b_high << (lo + T)) + (((w * HWS[T]) << R) << lo)).reshape(-1)


def _wave_cut(T, lo, a_count, bases=None):
    """Some wave's rows base + (k << lo), k < HWS 2^R, lie on both sides of the
    limit: its first row is below a_count and its last one is not."""
    if bases is None:  # (tiles up to one past the limit's)
        bases = _wave_bases(T, lo, (a_count >> (lo + T)) + 2)
    last = bases + (((HWS[T] << R) - 1) << lo)
    return bool(((bases < a_count) & (a_count <= last)).any())


@pytest.mark.parametrize("T", [7, 8])
def test_launch_rule_matches_wave_model(T):
    sb = 1024
    for lo in range(9):
        bases = _wave_bases(T, lo)
        span = (HWS[T] << R) << lo  # rows from a wave's first row to the next wave's
        rows = B_HIGH << (lo + T)
        cand = set(range(0, 80)) | {1 << lo, (1 << lo) + 1}
        for j in (1, 2, 3, 5, (1 << (T - R)) // HWS[T], rows // span - 1):
            for d in (-(1 << lo), -1, 0, 1, 1 << lo, span // 2, span - 1):
                cand.add(j * span + d)
        out = PassConsts()
        for a_count in sorted(c for c in cand if 0 <= c < rows):
            assert lib().rs16_host_pass_consts_rows(_prog("ENC_FIRST"), T, lo, sb, sb, sb, sb, sb // 8, 0, 0, 0, a_count, 0,
                                                    C.byref(out))
            assert (out.row_sets, out.reg_bits, out.load_shb) == (HWS[T], R, 0)
            assert out.voff32 == 1
            assert out.late_rows == (0 if _wave_cut(T, lo, a_count, bases) else 1), (T, lo, a_count)
            # the row limit is the gather's alone: the other programs ignore it
            for prog in ("ENC_MID", "ENC_LAST"):
                assert lib().rs16_host_pass_consts_rows(_prog(prog), T, lo, sb, sb, sb, sb, sb // 8, 0, 0, 0, a_count, 0,
                                                        C.byref(out))
                assert out.late_rows == 1, (prog, T, lo, a_count)
