"""Tower form of the work rows (rs16_tables.cpp,
rs16_gf.hpp tower_conv / mul_xor_tower_narrow), on the host: no device needed.

With beta = v_8 of the Cantor basis, v_{8+i} = a_i + v_i beta with a_i in the
GF(2^8) subfield span(v_0 .. v_7).  An element (lo, hi) is then a + b beta with
b = hi and a = lo ^ B(hi), B the bit matrix with columns a_i, and conv(lo, hi) =
(lo ^ B(hi), hi) switches between the two forms.  In tower form a subfield
constant c multiplies a and b by one byte map.  Checked here against the
oracle's multiply for all 65536 elements:

  - conv is an involution and leaves the high byte alone;
  - the a_i the tables derived reproduce v_{8+i}, and are the values the
    algebra gives for the polynomial 0x1002D;
  - for every subfield twiddle the middle passes of the paired sequences can
    stage (2^14- and 2^15-row chunks, skew 0 and the chunk size), dwords 0, 1,
    4, 5 and 16 of its tower table, applied to both bytes as v_perm would,
    equal conv(c * conv(e)); so does the library's 6-lookup multiply, and the
    12-lookup one on the same table;
  - the wide twiddles of those passes (one layer per direction of a 2^15-row
    chunk), sampled with the lowest and highest index of the layer, through the
    12-lookup multiply;
  - which sequences take the form: the paired ones, unless RS16_DIAG_NO_TOWER_ROWS.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import lib

A_I = [0x00, 0xCF, 0xAB, 0x21, 0x8A, 0x9D, 0x27, 0x1F]  # 


def _to_shard(e):
    """uint16 elements (a multiple of 32) -> shard bytes: per 64-byte block 32 low bytes, then 32 high bytes."""
    b = np.empty((e.size // 32, 2, 32), np.uint8)
    v = e.reshape(-1, 32)
    b[:, 0, :] = v & 0xFF
    b[:, 1, :] = v >> 8
    return b.reshape(-1)


def _from_shard(s):
    b = s.reshape(-1, 2, 32).astype(np.uint16)
    return (b[:, 0, :] | (b[:, 1, :] << 8)).reshape(-1)


ALL = np.arange(65536, dtype=np.uint16)


def _basis():
    return [lib().rs16_host_tower_basis(i) for i in range(8)]


def _conv_ref(e, a):
    """conv from its definition: lo ^= XOR of a_i over the set bits i of hi."""
    out = e.copy()
    for i in range(8):
        out ^= np.where((e >> (8 + i)) & 1, np.uint16(a[i]), np.uint16(0))
    return out


def _conv_lib(e):
    src = _to_shard(e)
    dst = np.empty_like(src)
    lib().rs16_host_tower_conv(src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), src.size)
    return _from_shard(dst)


def _oracle_mul(e, log_m):
    s = _to_shard(e).copy()
    O.mul(s, int(log_m))
    return _from_shard(s)


def test_basis_form():
    a = _basis()
    assert lib().rs16_host_tower_basis(8) == 0xFFFFFFFF
    assert all(x < 256 for x in a)
    log = O.table("log")
    beta = int(log[1 << 8])
    v_lo = np.zeros(32, np.uint16)
    v_lo[:8] = 1 << np.arange(8)
    prod = _oracle_mul(v_lo, beta)[:8]  # v_i * v_8 by the oracle
    for i in range(8):
        assert int(prod[i]) ^ a[i] == 1 << (8 + i), (i, hex(a[i]), hex(int(prod[i])))
    assert a == A_I


def test_conv_involution():
    got = _conv_lib(ALL)
    assert np.array_equal(got, _conv_ref(ALL, _basis()))
    assert np.array_equal(got >> 8, ALL >> 8)
    assert np.array_equal(_conv_lib(got), ALL)
    # a subfield element (c < 256) is exactly an element with b = 0, and conv fixes it
    assert np.array_equal(got[:256], ALL[:256]) and ((got < 256) == (ALL < 256)).all()


def _layer_indices(L, skew):
    """{layer kb: skew indices} the middle pass of a 2^L-row chunk stages for the direction at skew delta `skew`
    (TwiddleEntry, rs16_pass.hpp: lo = L // 2, T = L - lo, b_high = 0)."""
    lo, T = L // 2, L - L // 2
    out = {}
    for kb in range(T):
        d = 1 << (lo + kb)
        out[kb] = [g + d + skew - 1 for g in range(0, 1 << L, 2 * d)]
    return out


def _table(idx):
    t = (C.c_uint32 * 20)()
    assert lib().rs16_host_tower_twiddle(idx, t) == 1
    return np.frombuffer(t, np.uint32).copy()


def _byte_map(t):
    """The byte map of dwords 0, 1, 4, 5, 16 as three v_perm lookups of a byte's bit groups 0-2, 3-5, 6-7."""
    p0 = np.frombuffer(t[[0, 1]].tobytes(), np.uint8)
    p1 = np.frombuffer(t[[4, 5]].tobytes(), np.uint8)
    p2 = np.frombuffer(t[[16]].tobytes(), np.uint8)
    x = np.arange(256)
    return (p0[x & 7] ^ p1[(x >> 3) & 7] ^ p2[x >> 6]).astype(np.uint16)


def _mul_tower(e, idx, narrow):
    src = _to_shard(e)
    dst = np.empty_like(src)
    lib().rs16_host_mul_tower(src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), src.size, idx, narrow)
    return _from_shard(dst)


@pytest.fixture(scope="module")
def conv_all():
    return _conv_lib(ALL)


def _want(idx, conv_all, skew, a):
    if skew[idx] == 65535:  # the "no multiply" sentinel: the all-zero table
        return np.zeros(65536, np.uint16)
    return _conv_ref(_oracle_mul(conv_all, skew[idx]), a)


@pytest.mark.parametrize("L", [14, 15])
def test_tower_tables(L, conv_all):
    skew, a = O.table("skew"), _basis()
    narrow_seen = wide_seen = 0
    for delta in (0, 1 << L):
        for kb, idxs in _layer_indices(L, delta).items():
            narrow = [bool(lib().rs16_host_twiddle_narrow(i)) for i in idxs]
            assert len(set(narrow)) == 1, (L, delta, kb)  # a layer is narrow or wide as a whole
            if narrow[0]:
                pick = idxs
            else:  # sampled: the lowest and highest index of the layer, and a few between
                pick = sorted({idxs[0], idxs[-1], *idxs[1:-1:max(1, len(idxs) // 6)]})
            for idx in pick:
                want = _want(idx, conv_all, skew, a)
                assert np.array_equal(_mul_tower(ALL, idx, 0), want), (L, delta, kb, idx)
                if not narrow[0]:
                    wide_seen += 1
                    continue
                narrow_seen += 1
                assert np.array_equal(_mul_tower(ALL, idx, 1), want), (L, delta, kb, idx)
                m = _byte_map(_table(idx))
                assert np.array_equal(m[ALL & 0xFF] | (m[ALL >> 8] << 8), want), (L, delta, kb, idx)
    # 2^14: every layer of both directions narrow; 2^15: one wide layer (the one at skew 2^15)
    assert narrow_seen == (2 * 127 if L == 14 else 2 * 255 - 128)
    assert (wide_seen > 0) == (L == 15)


def test_which_sequences():
    f = lib().rs16_host_tower_rows
    p = lib().rs16_host_paired_rows
    for chunk in (8192, 16384, 32768):
        for sb in (64, 512, 960, 1024):
            for a_count in (chunk, chunk - 16, chunk - 8):
                for diag in (0, rs16.DIAG_NO_TOWER_ROWS, rs16.DIAG_NO_PAIRED_ROWS, rs16.DIAG_WIDE_TWIDDLES,
                             rs16.DIAG_NO_LATE_ROWS):
                    paired = p(chunk, sb, sb, a_count, 0, 0, diag)
                    want = int(bool(paired) and not diag & rs16.DIAG_NO_TOWER_ROWS)
                    assert f(chunk, sb, sb, a_count, 0, 0, diag) == want, (chunk, sb, a_count, diag)
    assert f(32768, 1024, 1024, 32768, 0, 0, 0) == 1 and f(16384, 512, 512, 16384, 16384, 16384, 0) == 1
    assert f(32768, 1024, 1024, 32768, 0, 0, rs16.DIAG_NO_TOWER_ROWS) == 0
    assert p(32768, 1024, 1024, 32768, 0, 0, rs16.DIAG_NO_TOWER_ROWS) == 1  # (the paired form stays)
