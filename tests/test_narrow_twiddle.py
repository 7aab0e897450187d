"""Subfield ("narrow") twiddles, CPU only (rs16_gf.hpp mul_xor_narrow,
rs16_internal.hpp twiddle_narrow).

The field elements are Cantor-basis coordinates, so an element < 256 lies in
the GF(2^8) subfield, and multiplying by one never carries an input's low
byte into the output's high byte: the middle passes leave those three of
the twelve table lookups out in the layers whose twiddles all are such
elements.  Which ones are is decided by an index rule (x = index + 1, b its
lowest set bit: x < 2^(b+8)).  Checked here from the library's own tables:

- the rule equals "twiddle < 256" for every skew index, and the twiddles are
  the reference's (oracle tables: exp[skew[i]], src/engine/tables.rs:164-205);
- the five table dwords the narrow multiply ignores are zero exactly there;
- the narrow multiply equals the full one and the oracle's NoSimd::mul for
  subfield multipliers, and differs for the others (so the test can fail).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
from rs16._lib import lib

N = 65535
IGNORED = [2, 3, 6, 7, 17]  # hi-output pools of the groups L0-2, L3-5, L6-7


@pytest.fixture(scope="module")
def twiddles():
    """(value, log, table[20], rule) of every skew index, from the library."""
    L = lib()
    val = np.empty(N, np.uint32)
    log = np.empty(N, np.uint32)
    tab = np.empty((N, 20), np.uint32)
    rule = np.empty(N, bool)
    lg = C.c_uint32()
    row = (C.c_uint32 * 20)()
    for i in range(N):
        val[i] = L.rs16_host_twiddle(i, C.byref(lg), row)
        log[i] = lg.value
        tab[i] = row
        rule[i] = L.rs16_host_twiddle_narrow(i)
    return val, log, tab, rule


def test_twiddles_are_the_references(twiddles):
    val, log, _, _ = twiddles
    skew, exp = O.table("skew"), O.table("exp")
    assert np.array_equal(log, skew)
    want = np.where(skew == 65535, 0, exp[skew])
    assert np.array_equal(val, want)
    assert lib().rs16_host_twiddle(N, None, None) == 2**32 - 1


def test_index_rule_is_value_below_256(twiddles):
    val, _, _, rule = twiddles
    x = np.arange(1, N + 1, dtype=np.int64)
    low = x & -x
    assert np.array_equal(rule, x < low * 256)  # the rule as stated
    assert np.array_equal(rule, val < 256)
    assert int(rule.sum()) == 1279


def test_ignored_pools_are_zero_exactly_for_narrow(twiddles):
    _, _, tab, rule = twiddles
    zero = (tab[:, IGNORED] == 0).all(axis=1)
    assert np.array_equal(zero, rule)


def _mul(fn, x, log_m):
    got = np.empty_like(x)
    fn(x.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p), x.size, log_m)
    return got


def test_narrow_multiply_matches_full_and_oracle():
    L = lib()
    log = O.table("log")
    rng = np.random.default_rng(256)
    x = rng.integers(0, 256, 64 * 16, dtype=np.uint8)  # 128 random quads
    # logs of the subfield elements 1 .. 255 (log 0 is the element 1), and
    # 65535, which multiplies by 1 as well (src/engine/tables.rs:70-76)
    narrow = sorted({int(log[c]) for c in range(1, 256)} | {0, 65535})
    assert narrow[0] == 0 and len(narrow) == 256
    for log_m in narrow:
        want = x.copy()
        O.mul(want, log_m, "nosimd")
        assert np.array_equal(_mul(L.rs16_host_mul, x, log_m), want), log_m
        assert np.array_equal(_mul(L.rs16_host_mul_narrow, x, log_m), want), log_m


def test_narrow_multiply_differs_for_wide_multipliers():
    L = lib()
    log = O.table("log")
    rng = np.random.default_rng(257)
    x = rng.integers(1, 256, 64 * 16, dtype=np.uint8)
    for c in (256, 257, 0x1234, 0x8000, 0xFFFF):
        log_m = int(log[c])
        want = x.copy()
        O.mul(want, log_m, "nosimd")
        assert np.array_equal(_mul(L.rs16_host_mul, x, log_m), want)
        assert not np.array_equal(_mul(L.rs16_host_mul_narrow, x, log_m), want), c
