"""References and helpers for the delta update's tests (rs16_update.hip,
DESIGN.md 3.15).  TEST INFRASTRUCTURE, like oracle_bind.py.

Two bit-exact references of  rec[j] ^= sum_e M[j][indices[e]] . delta_e :

  (a) the oracle's encode of the stripe after the overwrite (the tests call
      oracle_bind.encode themselves);
  (b) table_update(): the sum itself on 16-bit field elements, in numpy from the
      oracle's exp / log tables.  It never runs an encode on the data, so the
      recovery rows may hold any bytes (an update is linear, it does not ask
      for a codeword).

Element i of a 64-byte block is  byte[i] | byte[32 + i] << 8  (the shard
layout of the encode, src/engine.rs "shard data layout").
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from functools import lru_cache

import numpy as np

import oracle_bind as O
from rs16._lib import lib

GF_MODULUS = 65535
UpdateConsts = namedtuple("UpdateConsts", "quads_per_lane nslab rows_per_wave blocks")


def update_consts(rows, shard_bytes, n):
    """rs16_host_update_consts: the shape of the launch rs16_update_device
    makes for `rows` rows of `shard_bytes` and n deltas, or None."""
    q, ns, rpw, nb = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    ok = lib().rs16_host_update_consts(rows, shard_bytes, n, C.byref(q), C.byref(ns), C.byref(rpw), C.byref(nb))
    return UpdateConsts(q.value, ns.value, rpw.value, nb.value) if ok else None


@lru_cache(maxsize=None)
def _tables():
    return O.table("exp").astype(np.uint16), O.table("log").astype(np.int64)


def elements(rows):
    """(r, S) bytes -> (r, S / 2) uint16 field elements, block by block."""
    r, S = rows.shape
    b = rows.reshape(r, S // 64, 2, 32).astype(np.uint16)
    return (b[:, :, 0, :] | (b[:, :, 1, :] << 8)).reshape(r, S // 2)


def to_bytes(el):
    """The inverse of elements()."""
    r, half = el.shape
    e = el.reshape(r, half // 32, 1, 32)
    return np.concatenate([e & 0xFF, e >> 8], axis=2).astype(np.uint8).reshape(r, half * 2)


def gf_mul(c, x):
    """Elementwise product of uint16 field elements (broadcasting)."""
    exp, log = _tables()
    c, x = np.asarray(c, np.uint16), np.asarray(x, np.uint16)
    prod = exp[(log[c] + log[x]) % GF_MODULUS]
    return np.where((c != 0) & (x != 0), prod, np.uint16(0)).astype(np.uint16)


def table_update(rec, coef, delta):
    """rec (r, S) bytes ^ sum_e coef[:, e] . delta[e]: coef (r, n) uint16,
    delta (n, S) bytes.  Returns new bytes; the arguments stay as they are."""
    acc = elements(rec)
    d = elements(delta)
    for e in range(delta.shape[0]):
        acc = acc ^ gf_mul(coef[:, e:e + 1], d[e][None, :])
    return to_bytes(acc)


def unit_coefficients(k, m, indices, rate="default"):
    """(m, n) uint16 [j, e] = M[j][indices[e]], by the oracle's encode of unit
    vectors: the 32 elements of a block are independent codewords."""
    unit = np.zeros((k, 64), np.uint8)
    for e, i in enumerate(indices):
        unit[i, e] = 1
    rec = O.encode(k, m, unit, rate=rate)
    return (rec[:, :32].astype(np.uint16) | (rec[:, 32:].astype(np.uint16) << 8))[:, :len(indices)]


def edge_indices(k, n, seed):
    """n distinct originals, unsorted, with k - 1 first and (n >= 2) 0 last."""
    rng = np.random.default_rng(seed)
    mid = rng.permutation(np.arange(1, k - 1))[:max(n - 2, 0)].tolist()
    return ([k - 1] + [int(i) for i in mid] + [0])[:n] if n > 1 else [k - 1]
