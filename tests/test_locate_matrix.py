"""What rs16_locate_device (include/rs16.h) rests on, pinned on the CPU oracle,
and the brute-force reference locator the GPU tests import.

The encode is linear per element position: recovery_j = sum_i M[j][i]
original_i.  M comes from the oracle's encode of unit vectors.  Locating one
corrupt original from the ratio syndrome_0 / syndrome_1 needs M without a zero
entry and the k ratios M[0][i] / M[1][i] pairwise distinct (every 2 x 2 minor of
an MDS code's M is nonzero): pinned here for both rates and the multi-chunk
forms.

ref_locate() is the reference: syndromes from the oracle's encode, and per dirty
element every single-shard explanation -- recovery shard j (exactly syndrome_j
nonzero) or original i with error e (syndrome_j == M[j][i] e for ALL m rows: e
follows from row 0, candidates that miss row 1 are out, the others are checked
against every row).  Block status by the header's definitions.
"""
import functools

import numpy as np
import pytest

import oracle_bind as O

CLEAN, ORIGINAL, RECOVERY, UNLOCATABLE = 0, 1, 2, 3
NO_SHARD = 0xFFFFFFFF
MOD = 65535


@functools.lru_cache(maxsize=None)
def tables():
    return O.table("log").astype(np.int64), O.table("exp").astype(np.uint16)


def gf_mul(a, b):
    """Elementwise product of uint16 field elements (broadcasting)."""
    log, exp = tables()
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    p = exp[(log[a] + log[b]) % MOD]
    return np.where((a == 0) | (b == 0), np.uint16(0), p)


def gf_div(a, b):
    """a / b for nonzero b."""
    log, exp = tables()
    a, b = np.asarray(a, np.uint16), np.asarray(b, np.uint16)
    assert np.all(b != 0)
    return np.where(a == 0, np.uint16(0), exp[(log[a] - log[b]) % MOD])


def elements(shards):
    """(rows, S) uint8 -> (rows, S / 2) uint16: element p of a row is element p % 32
    of block p // 32, low byte at 64 (p // 32) + p % 32, high byte 32 further."""
    b = shards.reshape(shards.shape[0], -1, 2, 32).astype(np.uint16)
    return (b[:, :, 0, :] | b[:, :, 1, :] << 8).reshape(shards.shape[0], -1)


def element_bytes(e):
    """(..., 32) uint16 elements of blocks -> (..., 64) uint8 in the shard layout."""
    e = np.asarray(e, np.uint16)
    return np.concatenate([(e & 0xFF).astype(np.uint8), (e >> 8).astype(np.uint8)], axis=-1)


@functools.lru_cache(maxsize=None)
def matrix(k, m, rate="default"):
    """M as (m, k) uint16, from the oracle's encode of unit vectors: original i
    carries the element 1 at element position i."""
    sb = 64 * ((k + 31) // 32)
    unit = np.zeros((k, sb), np.uint8)
    i = np.arange(k)
    at = 64 * (i // 32) + i % 32
    unit[i, at] = 1
    rec = O.encode(k, m, unit, rate)
    M = rec[:, at].astype(np.uint16) | rec[:, at + 32].astype(np.uint16) << 8
    M.setflags(write=False)
    return M


def ref_locate(k, m, original, recovery, rate="default"):
    """(status uint8 [B], shard uint32 [B], fix uint8 [B, 64]) of a stored stripe."""
    log, exp = tables()
    M = matrix(k, m, rate)
    sb = original.shape[1]
    B = sb // 64
    syn = elements(O.encode(k, m, np.ascontiguousarray(original), rate) ^ recovery)  # (m, S / 2)
    nz = syn != 0
    count = nz.sum(axis=0)
    status = np.zeros(B, np.uint8)
    shard = np.full(B, NO_SHARD, np.uint32)
    fix = np.zeros((B, 64), np.uint8)
    # per dirty element: (kind, shard, error) or None
    found = {}
    dirty = np.flatnonzero(count)
    # recovery explanations: exactly one nonzero syndrome
    for p in dirty[count[dirty] == 1]:
        j = int(np.flatnonzero(nz[:, p])[0])
        found[int(p)] = (RECOVERY, j, int(syn[j, p]))
    # original explanations: every syndrome nonzero and syndrome_j == M[j][i] e for all j
    cand = dirty[count[dirty] == m]
    if cand.size:
        s0, s1 = syn[0, cand], syn[1, cand]
        e = exp[(log[s0][:, None] - log[M[0]][None, :]) % MOD]  # (n, k): the error original i would need
        hit = gf_mul(M[1][None, :], e) == s1[:, None]
        ns, js = np.nonzero(hit)
        full = (gf_mul(M[:, js], e[ns, js][None, :]) == syn[:, cand[ns]]).all(axis=0)  # against every row
        for n, i in zip(ns[full], js[full]):
            p = int(cand[n])
            assert p not in found, "two single-shard explanations of one element"
            found[p] = (ORIGINAL, int(i), int(e[n, i]))
    by_block = {}
    for p in dirty:
        by_block.setdefault(int(p) // 32, []).append(int(p))
    for c, ps in by_block.items():
        ex = [found.get(p) for p in ps]
        if any(x is None for x in ex) or len({(x[0], x[1]) for x in ex}) != 1:
            status[c] = UNLOCATABLE
            continue
        status[c], shard[c] = ex[0][0], ex[0][1]
        el = np.zeros(32, np.uint16)
        for p, x in zip(ps, ex):
            el[p % 32] = x[2]
        fix[c] = element_bytes(el)
    return status, shard, fix


# the shapes and rates the feature was reasoned about (both rates, the multi-chunk forms)
SHAPES = [(5, 3, "high"), (3, 5, "low"), (100, 7, "default"), (40, 70, "default"), (300, 2, "high"),
          (2, 300, "low"), (1000, 1000, "default"), (3000, 1000, "high"), (300, 2000, "low"),
          (4096, 2, "default"), (2, 2, "default"), (1, 2, "default")]


@pytest.mark.parametrize("k,m,rate", SHAPES)
def test_matrix_has_no_zero_and_distinct_ratios(k, m, rate):
    log, _ = tables()
    M = matrix(k, m, rate)
    assert M.shape == (m, k)
    assert (M != 0).all(), "M has a zero entry"
    ratio = (log[M[0]] - log[M[1]]) % MOD
    assert np.unique(ratio).size == k, "two originals share M[0][i] / M[1][i]"


def test_matrix_is_the_encode():
    # recovery == M x original, per element
    k, m = 5, 3
    rng = np.random.default_rng(1)
    original = rng.integers(0, 256, (k, 128), dtype=np.uint8)
    want = elements(O.encode(k, m, original))
    M = matrix(k, m)
    got = np.zeros_like(want)
    o = elements(original)
    for i in range(k):
        got ^= gf_mul(M[:, i][:, None], o[i][None, :])
    assert np.array_equal(got, want)


def test_ref_locate_on_constructed_stripes():
    k, m, sb = 5, 3, 192
    rng = np.random.default_rng(2)
    original = rng.integers(0, 256, (k, sb), dtype=np.uint8)
    recovery = O.encode(k, m, original)
    st, sh, fx = ref_locate(k, m, original, recovery)
    assert not st.any() and (sh == NO_SHARD).all() and not fx.any()
    # an original in block 0, a recovery shard in block 2, two originals in block 1
    o, r = original.copy(), recovery.copy()
    o[3, 7] ^= 0x10
    o[3, 32 + 9] ^= 0x01
    r[2, 128 + 40] ^= 0x80
    o[0, 64 + 1] ^= 1
    o[4, 64 + 2] ^= 1
    st, sh, fx = ref_locate(k, m, o, r)
    assert st.tolist() == [ORIGINAL, UNLOCATABLE, RECOVERY]
    assert sh.tolist() == [3, NO_SHARD, 2]
    assert np.array_equal(fx[0], o[3, :64] ^ original[3, :64])
    assert not fx[1].any()
    assert np.array_equal(fx[2], r[2, 128:] ^ recovery[2, 128:])
    # two originals at one element with m = 3: unlocatable, never a third shard
    o = original.copy()
    o[0, 5] ^= 1
    o[1, 5] ^= 2
    st, sh, _ = ref_locate(k, m, o, recovery)
    assert st.tolist() == [UNLOCATABLE, CLEAN, CLEAN]
