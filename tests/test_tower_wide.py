"""The wide multiplies of the tower form (rs16_gf.hpp
mul_xor_tower_wide / mul_xor_tower_beta), on the host: no device needed.

With beta = v_8 and beta^2 = beta + v_7 a constant c = c0 + c1 beta acts on x =
a + b beta as (a c0 + b c1 v_7) + (a c1 + b c0 + b c1) beta.  Three of the four
byte maps of c's tower table do: P1 = M_{c0}(a), Q = M_{c1 v_7}(b), P3 =
M_{c0 ^ c1}(a ^ b), product (P1 ^ Q, P3 ^ P1) -- 9 lookups, the multiply of the
T = 7 passes.  With c1 = 1 (the one wide layer of a 2^15-row chunk's middle
pass) the product is (M_{c0}(a) ^ M_{v_7}(b), M_{c0}(b) ^ a ^ b).  Checked
against the oracle's multiply, through the host hooks tests/test_tower_form.py
uses (the kernels' code with v_perm emulated):

  - beta^2 = beta ^ v_7;
  - every twiddle the T = 7 passes of a 16384:16384 and a 32768:32768 stripe
    stage, in both directions (skew 0 and the stripe's size; the IFFT and the
    FFT of one skew stage the same tables), 65024 indices, each over all 65536
    elements: the oracle multiplies, the library's compiled loop
    (rs16_host_tower_sweep) multiplies in tower form, converts and compares;
  - the lowest, the highest and some indices between of every layer, skew and
    size again through the one-index hook, with the 12-lookup multiply beside;
  - the 128 twiddles of the middle pass's wide layer, all 65536 elements each,
    through the c1 = 1 multiply, the three-map one and the 12-lookup one; their
    tables' L -> hi map is the identity (c1 = 1).
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
from rs16._lib import lib

from test_tower_form import ALL, _conv_lib, _conv_ref, _basis, _mul_tower, _oracle_mul, _table, _to_shard

WIDE3, BETA = 2, 3  # rs16_host_mul_tower's forms


def _t7_indices(L, skew):
    """{layer kb: skew indices} of the first / last pass of a 2^L-row chunk at skew delta `skew` (TwiddleEntry,
    rs16_pass.hpp: lo = 0, T = L // 2, tiles b_high < 2^(L - T))."""
    T = L // 2
    return {kb: [g + (1 << kb) + skew - 1 for g in range(0, 1 << L, 2 << kb)] for kb in range(T)}


def _want(x_tower, log_m, a):
    if log_m == 65535:  # the "no multiply" sentinel: the all-zero table
        return np.zeros(x_tower.size, np.uint16)
    return _conv_ref(_oracle_mul(_conv_ref(x_tower, a), log_m), a)


def test_beta_squared():
    log = O.table("log")
    e = np.zeros(32, np.uint16)
    e[0] = 1 << 8
    assert int(_oracle_mul(e, int(log[1 << 8]))[0]) == (1 << 8) ^ (1 << 7)


def _sweep(idxs, form, skew, shard_in, tower_in):
    """Elements that differ, over the indices idxs, between the oracle's products of shard_in (bytes, the oracle's
    coordinates) and the library's of tower_in (the same elements in tower form), in batches of 256 indices."""
    want = np.zeros((256, shard_in.size), np.uint8)
    bad = 0
    for i in range(0, len(idxs), 256):
        part = np.asarray(idxs[i:i + 256], np.uint32)
        for j, idx in enumerate(part):
            lm = int(skew[idx])
            if lm == 65535:  # the "no multiply" sentinel: the all-zero table
                want[j] = 0
            else:
                np.copyto(want[j], shard_in)
                O.mul(want[j], lm)
        bad += lib().rs16_host_tower_sweep(part.ctypes.data_as(C.POINTER(C.c_uint32)), part.size, form,
                                           tower_in.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p),
                                           shard_in.size)
    return bad


def test_every_t7_twiddle_all_elements():
    # (a 16384-row stripe's indices, x < 16384 and 16384 < x < 32768, are among those of a 32768-row stripe's skew 0)
    skew, a = O.table("skew"), _basis()
    small = set(sum(_t7_indices(14, 0).values(), []) + sum(_t7_indices(14, 1 << 14).values(), []))
    idxs = sum(_t7_indices(15, 0).values(), []) + sum(_t7_indices(15, 1 << 15).values(), [])
    assert small <= set(idxs) and len(set(idxs)) == len(idxs) == 2 * (32768 - 256)  # every x - 1, x no multiple of 128
    tower_in, shard_in = _to_shard(ALL), _to_shard(_conv_ref(ALL, a))
    assert _sweep(idxs, WIDE3, skew, shard_in, tower_in) == 0
    # the sweep does tell: the c1 = 1 form is wrong for these twiddles, and a shifted index is another constant
    assert _sweep(idxs[:4], BETA, skew, shard_in, tower_in) > 0
    assert _sweep([i + 2 for i in idxs[5:9]], WIDE3, np.roll(skew, 2), shard_in, tower_in) > 0  # (the oracle: index i)


@pytest.mark.parametrize("L", [14, 15])
def test_t7_twiddles_all_elements(L):
    assert L // 2 == 7
    skew, a = O.table("skew"), _basis()
    for delta in (0, 1 << L):
        for kb, idxs in _t7_indices(L, delta).items():
            for idx in sorted({idxs[0], idxs[-1], *idxs[1:-1:max(1, len(idxs) // 4)]}):
                want = _want(ALL, int(skew[idx]), a)
                assert np.array_equal(_mul_tower(ALL, idx, WIDE3), want), (L, delta, kb, idx)
                assert np.array_equal(_mul_tower(ALL, idx, 0), want), (L, delta, kb, idx)


def test_conversion_at_the_edges():
    """The first pass's first butterfly, y ^= x, x ^= y c, with both rows converted between its two halves, and the
    last pass's last, x ^= y c, y ^= x, converted after the multiply: tower form on Z's side, shard coordinates on
    the caller's, as conv(x) c computed in tower form is conv of the oracle's x c."""
    skew, a = O.table("skew"), _basis()
    rng = np.random.default_rng(15)
    x, y = rng.integers(0, 65536, 4096).astype(np.uint16), rng.integers(0, 65536, 4096).astype(np.uint16)
    for idx in (2, 32768 + 4, 100, 65000):
        lm = int(skew[idx])
        # IFFT, shard in, tower out
        y1 = y ^ x
        x1 = x ^ _oracle_mul(y1, lm)
        ty, tx = _conv_lib(y1), _conv_lib(x)
        tx = tx ^ _mul_tower(ty, idx, WIDE3)
        assert np.array_equal(_conv_lib(tx), x1) and np.array_equal(_conv_lib(ty), y1)
        # FFT, tower in, shard out: conv(y) ^ conv(x') = conv(y ^ x')
        x2 = x ^ _oracle_mul(y, lm)
        tx = _conv_lib(x) ^ _mul_tower(_conv_lib(y), idx, WIDE3)
        assert np.array_equal(_conv_lib(tx), x2)
        assert np.array_equal(_conv_lib(_conv_lib(y)) ^ _conv_lib(tx), y ^ x2)


def test_mid_wide_layer():
    skew, a = O.table("skew"), _basis()
    L, lo = 15, 7
    ident = np.array([0x03020100, 0x07060504, 0x18100800, 0x38302820, 0xC0804000], np.uint32)
    idxs = [g + (1 << lo) + (1 << L) - 1 for g in range(0, 1 << L, 2 << lo)]
    assert len(idxs) == 128
    for idx in idxs:
        assert not lib().rs16_host_twiddle_narrow(idx)
        assert np.array_equal(_table(idx)[[2, 3, 6, 7, 17]], ident), idx  # c1 = 1
        want = _want(ALL, int(skew[idx]), a)
        for form in (BETA, WIDE3, 0):
            assert np.array_equal(_mul_tower(ALL, idx, form), want), (idx, form)
    # a wide twiddle with another c1 does not take the c1 = 1 form
    other = (1 << L) + 1 - 1 + 2  # x = 2^15 + 2: layer 1, span(v_0 .. v_14)
    assert not np.array_equal(_table(other)[[2, 3, 6, 7, 17]], ident)
    want = _want(ALL, int(skew[other]), a)
    assert np.array_equal(_mul_tower(ALL, other, WIDE3), want)
    assert not np.array_equal(_mul_tower(ALL, other, BETA), want)
