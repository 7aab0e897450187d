"""The repair (rs16_repair_device, include/rs16.h) without a device.

1. The entry points and the host hook resolve in the library and the Python
   wrappers exist.
2. rs16_host_repair_path: the five answers, and the last pass's tile range at
   the three geometries where it differs in kind.
3. The algebra, on the oracle's engine ops alone.  The reference's decode
   (rate_high.rs:168-247, rate_low.rs:168-247; oracle/rs16_oracle.c rate_decode)
   computes FFT(FD(IFFT(received x e))) over all n work rows and then reveals
   -- multiplies by 65535 - e -- the lost originals only.  After the FFT the
   row of EVERY erased position holds the codeword's value there times the
   erasure multiplier, the erased recovery positions included: the reveal
   loop extended to the not-received rows of both segments gives back the
   recovery shards of the encoder bit for bit.  That is why the device path
   needs no new math, and these are the oracle ops it relies on.
"""
import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import lib
from rs16.util import generate_original

GF_ORDER, GF_MODULUS = 65536, 65535


def test_symbols_and_wrappers():
    for name in ("rs16_repair_device", "rs16_repair_device_batch", "rs16_host_repair_path"):
        assert hasattr(lib(), name), name
    for name in ("repair_device", "repair_device_batch", "repair_path"):
        assert callable(getattr(rs16, name)), name
    names = [lib().rs16_prog_name(p).decode() for p in range(lib().rs16_prog_count())]
    # appended: every earlier id keeps its name and place
    assert names[-3:] == ["DEC_LAST_ALL", "DEC_SINGLE_ALL", "REPAIR_COPY"]
    assert names[:12] == ["GEN_FFT", "GEN_IFFT", "ENC_FIRST", "ENC_MID", "ENC_LAST", "ENC_SINGLE", "DEC_FIRST",
                          "DEC_MID", "DEC_LAST", "DEC_SINGLE", "DEC_HALF_LAST", "DEC_HALF_SINGLE"]
    assert names[12:19] == ["DEC_HALF_FIRST", "DEC_HALF_MID", "EVAL_POLY", "COL_ENC", "COL_DEC", "DEC_MID_DIRECT",
                            "DEC_TILE_LAST"]


def test_path_choice():
    k, m = 100, 60
    assert rs16.repair_path(k, m, k, m) == (0, 0, 0, 0)          # everything received
    assert rs16.repair_path(k, m, k - 7, m) == (1, 0, 0, 0)      # originals only: the decode
    assert rs16.repair_path(k, m, k, m - 1) == (2, 0, 0, 0)      # recovery only: encode + copy
    assert rs16.repair_path(k, m, k - 1, m - 1)[0] == 3          # both kinds
    assert rs16.repair_path(k, m, k - 30, m - 30)[0] == 3        # exactly k received
    # the call fails: too few received, a count above its shard count, unsupported counts
    assert rs16.repair_path(k, m, k - 31, m - 30) == (-1, 0, 0, 0)
    assert rs16.repair_path(k, m, k + 1, m) == (-1, 0, 0, 0)
    assert rs16.repair_path(k, m, k, m + 1) == (-1, 0, 0, 0)
    assert rs16.repair_path(0, m, 0, m) == (-1, 0, 0, 0)
    assert rs16.repair_path(40000, 40000, 40000, 39999) == (-1, 0, 0, 0)
    # NULL outputs are allowed
    assert lib().rs16_host_repair_path(k, m, k - 1, m - 1, None, None, None) == 3


@pytest.mark.parametrize("k,m,rows,lo,first,tiles", [
    # one-pass kernel: one tile
    (100, 100, 256, 0, 0, 1),
    # recovery segment [0, 5), chunk 8, originals [8, 3008): 4096 work rows, 2^6-row
    # tiles, tile 0 holds rows of both segments: one range, ceil(3008 / 64) tiles
    (3000, 5, 4096, 6, 0, 47),
    # segments [0, 200) and [256, 456) of 512 rows, 2^4-row tiles: 13 + 13 tiles,
    # tiles 13 .. 15 (rows 208 .. 255, between the segments) left out
    (200, 200, 512, 4, 16, 26),
    # segments [0, 30000) and [32768, 62768), 2^8-row tiles: 118 + 118, tiles 118 .. 127 left out
    (30000, 30000, 65536, 8, 128, 236),
    # the segments touch: one range
    (32768, 32768, 65536, 8, 0, 256),
    # low rate: originals are segment A
    (5, 3000, 4096, 6, 0, 47),
])
def test_last_pass_tiles(k, m, rows, lo, first, tiles):
    high = rs16.use_high_rate(k, m)
    assert lib().rs16_decoder_work_count(1 if high else 0, k, m) == rows
    assert rs16.repair_path(k, m, k - 1, m - 1) == (3, lo, first, tiles)


# ---------------------------------------------------------------------------
# the algebra on the oracle
# ---------------------------------------------------------------------------
def oracle_repair(k, m, high, original, recovery, orig_ok, rec_ok):
    """rate_decode's sequence on the oracle's engine ops with the reveal loop
    over the not-received rows of both segments.  Returns (originals, recovery)
    with the lost rows filled in."""
    sb = original.shape[1]
    a, b = (recovery, original) if high else (original, recovery)
    a_ok, b_ok = (rec_ok, orig_ok) if high else (orig_ok, rec_ok)
    a_count, b_count = len(a), len(b)
    chunk = 1 << (a_count - 1).bit_length()
    end = chunk + b_count
    n = 1 << (end - 1).bit_length()
    received = np.zeros(n, bool)
    received[:a_count] = a_ok
    received[chunk:end] = b_ok
    er = np.zeros(GF_ORDER, np.uint16)
    er[:a_count] = ~received[:a_count]
    if high:
        er[a_count:chunk] = 1
    er[chunk:end] = ~received[chunk:end]
    if not high:
        er[end:] = 1
    O.eval_poly(er, end if high else GF_ORDER)
    w = np.zeros((n, sb), np.uint8)
    w[:a_count] = a
    w[chunk:end] = b
    w[~received] = 0
    for i in np.flatnonzero(received):
        O.mul(w[i], int(er[i]))
    O.ifft(w, 0, n, end, 0)
    O.formal_derivative(w)
    O.fft(w, 0, n, end, 0)
    lost = [i for i in list(range(a_count)) + list(range(chunk, end)) if not received[i]]
    for i in lost:
        O.mul(w[i], int(GF_MODULUS - er[i]))
    out_a, out_b = a.copy(), b.copy()
    for i in lost:
        if i < a_count:
            out_a[i] = w[i]
        else:
            out_b[i - chunk] = w[i]
    return (out_b, out_a) if high else (out_a, out_b)


SHAPES = [(3, 2), (100, 100), (300, 70), (70, 300), (1000, 100), (100, 1000), (5, 300), (300, 5), (600, 600)]


def _cases():
    for k, m in SHAPES:
        for tag, nlost in (("m", m), ("half", max(1, m // 2)), ("one", 1)):
            yield k, m, tag, nlost
    for k, m in ((100, 100), (300, 70), (70, 300)):
        yield k, m, "rec1", 0    # no original lost, one recovery shard lost
        yield k, m, "exact", 0   # exactly k received, both kinds lost


@pytest.mark.parametrize("k,m,tag,nlost", list(_cases()))
def test_algebra_on_oracle(k, m, tag, nlost):
    sb = 64
    rng = np.random.default_rng(1000 * k + m + len(tag))
    original = generate_original(k, sb, k + m)
    recovery = O.encode(k, m, original)
    ok = np.ones(k + m, bool)
    if tag == "rec1":
        ok[k + int(rng.integers(m))] = False
    elif tag == "exact":
        lost = rng.choice(k + m, m, replace=False)
        if (lost < k).all() or (lost >= k).all():
            lost[0] = 0 if (lost >= k).all() else k
        ok[np.unique(lost)] = False
    else:
        ok[rng.choice(k + m, nlost, replace=False)] = False  # at most m lost: at least k received
    assert ok.sum() >= k
    holes_o, holes_r = original.copy(), recovery.copy()
    holes_o[~ok[:k]] = 0xA5
    holes_r[~ok[k:]] = 0xA5
    high = bool(rs16.use_high_rate(k, m))
    got_o, got_r = oracle_repair(k, m, high, holes_o, holes_r, ok[:k], ok[k:])
    assert np.array_equal(got_o, original)
    assert np.array_equal(got_r, recovery)
