"""The delta update of recovery shards (rs16_update_plan)
rests on two facts about the reference encode (src/rate/rate_high.rs:44-83,
rate_low.rs:44-83), checked here on the oracle alone:

- it is GF(2^16)-linear per element position: recovery_j = sum_i M[j][i]
  original_i, so changing originals `indices` from old to new changes
  recovery_j by sum_e M[j][indices[e]] (old_e ^ new_e);
- the 32 elements of a 64-byte block are independent codewords
  (src/algorithm.md:18-32), so one encode of a k x 64 B stripe whose element e
  is the field element 1 in shard indices[e] and 0 elsewhere returns
  M[j][indices[e]] in element e of recovery row j.

For every geometry: the coefficients from the unit-vector encode, the update
applied with the oracle's multiply (NoSimd::mul, src/engine/engine_nosimd.rs:65-79)
at 128-byte shards, compared bit for bit with a full re-encode.  No
coefficient is zero (M is the parity part of an MDS code).
"""
import numpy as np
import pytest

import oracle_bind as O
from rs16.util import generate_original

# (k, m, rate, n)
CASES = [
    (1, 1, "default", 1),
    (3, 5, "default", 2),
    (5, 3, "low", 5),
    (100, 300, "default", 7),
    (300, 100, "default", 32),
    (513, 1024, "low", 3),
    (1000, 1000, "default", 32),
    (3000, 1000, "high", 5),  # multi-chunk
]


def unit_coefficients(k, m, indices, rate):
    """(m, n) uint16: M[j][indices[e]] from one encode of the unit-vector stripe."""
    unit = np.zeros((k, 64), np.uint8)
    for e, i in enumerate(indices):
        unit[i, e] = 1  # low byte 1, high byte 0: the field element 1
    rec = O.encode(k, m, unit, rate=rate)
    n = len(indices)
    return rec[:, :n].astype(np.uint16) | (rec[:, 32:32 + n].astype(np.uint16) << 8)


@pytest.mark.parametrize("k,m,rate,n", CASES, ids=[f"{k}:{m}-{r}-n{n}" for k, m, r, n in CASES])
def test_update_equals_reencode(k, m, rate, n):
    S = 128
    rng = np.random.default_rng(k * 7 + m)
    indices = sorted(rng.choice(k, n, replace=False).tolist())
    # first and last original take part where there is room
    if n >= 2:
        indices[0], indices[-1] = 0, k - 1
    coef = unit_coefficients(k, m, indices, rate)
    assert coef.all(), "a zero coefficient in the parity part of an MDS code"
    log = O.table("log")

    old = generate_original(k, S, 11)
    new = old.copy()
    new[indices] = rng.integers(0, 256, (n, S), dtype=np.uint8)
    delta = old[indices] ^ new[indices]
    rec = O.encode(k, m, old, rate=rate)
    for j in range(m):
        for e in range(n):
            t = delta[e].copy()
            O.mul(t, int(log[coef[j, e]]))
            rec[j] ^= t
    assert np.array_equal(rec, O.encode(k, m, new, rate=rate))
