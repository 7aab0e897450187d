"""Delta update (rs16_update_device, rs16_update.hip): every
kernel instantiation, row runs with their tails, edge deltas, and a freed
plan's address reused.  tests/test_gpu_update.py checks the plan's encode
paths and the API; this file is about what the kernel's code depends on.

update_kernel<N, Q> is 40 kernels (N = 1 .. 32 at Q = 1, N = 1 .. 8 at Q = 2),
each with its own schedule of table groups, and the launch's heuristics pick
the rows per wave.  Every case first asks rs16_host_update_consts (the function
the launcher calls; tests/test_update_launch_consts.py) what is about to run
and asserts the (N, Q, slabs, rows per wave, rows of the last run) it was
written for: a change of the heuristics fails the case instead of silently
moving it to another path.

References, both bit-exact (update_ref.py):
  (a) the oracle's encode of the stripe after the overwrite;
  (b) rec ^ sum_e coef[j, e] . delta_e in numpy from the oracle's exp / log
      tables, on recovery rows of random bytes (no codeword), with coef =
      plan.coefficients() asserted equal to the oracle's unit-vector encode.

Every buffer of recovery rows is  64 guard bytes | a guard row | the m rows |
a guard row | 64 guard bytes;  the guards and the rows outside
[pos, pos + cnt) must come back unchanged, and so must the deltas.
"""
from functools import lru_cache

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original
from update_ref import edge_indices, elements, table_update, to_bytes, unit_coefficients, update_consts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


def assert_form(plan, rows, S, N, Q, nslab, rows_per_wave, tail):
    """The kernel and launch shape the case was written for."""
    c = update_consts(rows, S, len(plan))
    got = (len(plan), c.quads_per_lane, c.nslab, c.rows_per_wave, rows % c.rows_per_wave)
    assert got == (N, Q, nslab, rows_per_wave, tail), f"(N, Q, slabs, rows per wave, tail) = {got}"
    return c


def make_stripe(k, m, S, rate="default", seed=1):
    """(old originals, their recovery rows by the oracle), read-only."""
    old = generate_original(k, S, seed)
    rec = O.encode(k, m, old, rate=rate)
    old.setflags(write=False)
    rec.setflags(write=False)
    return old, rec


stripe = lru_cache(maxsize=None)(make_stripe)  # the small shapes, shared among their cases


def random_rows(r, S, seed):
    return np.random.default_rng(seed).integers(0, 256, (r, S), dtype=np.uint8)


def apply_guarded(eng, plan, S, m, rec, delta, pos=0, cnt=None):
    """The update of rows [pos, pos + cnt) of rec (m, S) on the device, inside
    guards; asserts that the guards, the other rows and the deltas come back
    unchanged and returns the updated rows (cnt, S)."""
    cnt = m - pos if cnt is None else cnt
    edge = random_rows(1, 2 * (64 + S), 99).reshape(-1)
    buf = np.concatenate([edge[:64 + S], rec.reshape(-1), edge[64 + S:]])
    d_buf = DeviceArray.from_numpy(eng, buf)
    d_delta = DeviceArray.from_numpy(eng, delta)
    plan.apply(S, d_delta.ptr, d_buf.offset(64 + S + pos * S), recovery_pos=pos, recovery_n=cnt)
    got = d_buf.download()
    assert np.array_equal(d_delta.download(shape=delta.shape), delta), "the deltas were written"
    assert np.array_equal(got[:64 + S], edge[:64 + S]), "guard bytes / guard row before the rows"
    assert np.array_equal(got[-(64 + S):], edge[64 + S:]), "guard row / guard bytes behind the rows"
    rows = got[64 + S:-(64 + S)].reshape(m, S)
    assert np.array_equal(rows[:pos], rec[:pos]), "rows before the range"
    assert np.array_equal(rows[pos + cnt:], rec[pos + cnt:]), "rows behind the range"
    return rows[pos:pos + cnt]


def mismatch(got, want):
    """'' or where two (rows, S) arrays differ, for the assertion's message."""
    if np.array_equal(got, want):
        return ""
    r, b = np.nonzero(got != want)
    return (f"{len(r)} bytes differ in {len(np.unique(r))} of {got.shape[0]} rows; first (row, byte) "
            f"({r[0]}, {b[0]}), last ({r[-1]}, {b[-1]}); rows {np.unique(r)[:8]}, bytes {np.unique(b)[:8]}")


def check_both(eng, plan, k, m, S, indices, delta, coef, rate="default"):
    """References (a) and (b) over all m rows."""
    old, rec_old = stripe(k, m, S, rate)
    new = old.copy()
    new[indices] ^= delta
    got = apply_guarded(eng, plan, S, m, rec_old, delta)
    bad = mismatch(got, O.encode(k, m, new, rate=rate))
    assert not bad, "against the oracle's re-encode: " + bad
    junk = random_rows(m, S, 7)
    got = apply_guarded(eng, plan, S, m, junk, delta)
    bad = mismatch(got, table_update(junk, coef, delta))
    assert not bad, "against the table multiply: " + bad


def plan_with_coefficients(eng, k, m, indices, rate="default"):
    plan = rs16.UpdatePlan(k, m, indices, rate, engine=eng)
    coef = plan.coefficients()
    assert np.array_equal(coef, unit_coefficients(k, m, indices, rate)), "plan.coefficients() against the oracle"
    return plan, coef


# ---- 3a: every instantiation ----
# k = 40, m = 27: 27 rows x 2 slabs = 54 waves of one row, 14 workgroups, the last half full.
K, M = 40, 27
EVERY = [(1, n, 576) for n in range(1, 33)] + [(2, n, S) for S in (1600, 1088) for n in range(1, 9)]


def test_every_instantiation_is_listed():
    forms = set()
    for Q, n, S in EVERY:
        c = update_consts(M, S, n)
        assert c.quads_per_lane == Q
        forms.add((n, Q))
    assert forms == {(n, 1) for n in range(1, 33)} | {(n, 2) for n in range(1, 9)}


@pytest.mark.parametrize("Q,n,S", EVERY, ids=[f"Q{Q}-n{n}-{S}B" for Q, n, S in EVERY])
def test_every_instantiation(eng, Q, n, S):
    indices = edge_indices(K, n, 1000 * Q + n)
    plan, coef = plan_with_coefficients(eng, K, M, indices)
    c = assert_form(plan, M, S, N=n, Q=Q, nslab=2, rows_per_wave=1, tail=0)
    assert c.blocks == 14 and M * c.nslab == 54
    check_both(eng, plan, K, M, S, indices, random_rows(n, S, S + n), coef)
    plan.close()


# ---- 3b: row runs and their tails ----
# k, m, S, n, pos, cnt (None: all), Q, slabs, rows per wave, tail
RUNS = [
    (40, 32768, 64, 3, 5, 16385, 1, 1, 2, 1),
    (40, 32768, 64, 2, 0, 24577, 1, 1, 3, 1),
    (40, 32768, 64, 11, 8190, 24578, 1, 1, 3, 2),
    (4096, 61440, 64, 32, 45055, 16385, 1, 1, 2, 1),  # ends at the last row of the largest low-rate index array
    (40, 16385, 1024, 9, 0, None, 1, 2, 4, 1),
    (40, 8193, 1088, 5, 0, None, 2, 2, 2, 1),
    (33, 1540, 16448, 7, 0, None, 2, 17, 3, 1),
    (33, 1027, 33344, 13, 0, None, 1, 66, 8, 3),
    # the cap of 32 rows per wave needs rows x bytes >= 128 MiB: no smaller shape reaches it
    (33, 4099, 32768, 9, 0, None, 1, 64, 32, 3),
]


@pytest.mark.parametrize("k,m,S,n,pos,cnt,Q,nslab,rpw,tail", RUNS,
                         ids=[f"{r[0]}:{r[1]}x{r[2]}-n{r[3]}-rows{r[4]}+{r[5] or r[1]}" for r in RUNS])
def test_row_runs(eng, k, m, S, n, pos, cnt, Q, nslab, rpw, tail):
    cnt = m if cnt is None else cnt
    indices = edge_indices(k, n, m + n)
    plan = rs16.UpdatePlan(k, m, indices, engine=eng)
    assert_form(plan, cnt, S, N=n, Q=Q, nslab=nslab, rows_per_wave=rpw, tail=tail)
    if m * S >= 1 << 27:
        try:
            DeviceArray(eng, (m + 2) * S + 128)  # (freed at once)
        except rs16.Error as e:
            pytest.skip(f"no device memory for {m} rows of {S} B: {e}")
    old, rec_old = make_stripe(k, m, S)
    delta = random_rows(n, S, m + S)
    new = old.copy()
    new[indices] ^= delta
    got = apply_guarded(eng, plan, S, m, rec_old, delta, pos, cnt)
    plan.close()
    bad = mismatch(got, O.encode(k, m, new)[pos:pos + cnt])
    assert not bad, bad


# ---- 3c: delta contents ----
# S, n: two quads per lane with the selectors kept; one quad, kept; one quad, selectors per row
CONTENT_SHAPES = [(1600, 8), (576, 12), (576, 20)]
NIBBLES = np.array([v << (4 * p) for p in range(4) for v in range(16)], np.uint16)


def one_element(n, S, member, block, el, high):
    d = np.zeros((n, S), np.uint8)
    d[member, block * 64 + 32 * high + el] = 0xA7
    return d


def delta_cases(S, n):
    """(name, delta (n, S)) for one shape."""
    nblk = S // 64
    slab_blocks = 16 if S >= 1024 and n <= 8 else 8        # blocks of a slab: 64 Q quads of 8 bytes
    tail_block = (nblk - 1) // slab_blocks * slab_blocks   # the first column of the last, partial slab
    assert 0 < tail_block and nblk % slab_blocks != 0
    rnd = random_rows(n, S, 31 * S + n)
    yield "zero", np.zeros((n, S), np.uint8)
    some = rnd.copy()
    some[1::2] = 0
    some[n - 1] = 0
    yield "members-zero", some
    for high in (0, 1):
        for name, block, el in (("el0", 0, 0), ("el31", 0, 31), ("last-block", nblk - 1, 17), ("tail-slab", tail_block, 5)):
            yield f"one-{name}-{'high' if high else 'low'}", one_element(n, S, (n - 1, 1)[high], block, el, high)
    el = np.stack([np.resize(np.roll(NIBBLES, -e), S // 2) for e in range(n)])
    yield "nibbles", to_bytes(el)
    for v in (0xFFFF, 0x0001, 0x8000):
        yield f"all-{v:04x}", to_bytes(np.full((n, S // 2), v, np.uint16))
    yield "same-in-all", np.repeat(rnd[:1], n, axis=0)
    part = np.zeros((n, S), np.uint8)
    for e in range(n):
        a, b = 37 + e, S - 101 - 2 * e
        part[e, a:b] = rnd[e, a:b]
    yield "byte-range", part


CONTENTS = [(S, n, name) for S, n in CONTENT_SHAPES for name, _ in delta_cases(S, n)]


@pytest.fixture(scope="module")
def content_plans(eng):
    plans = {}
    for S, n in CONTENT_SHAPES:
        indices = edge_indices(K, n, S + n)
        plans[S, n] = (indices,) + plan_with_coefficients(eng, K, M, indices)
    yield plans
    for _, plan, _ in plans.values():
        plan.close()


def test_nibble_row_has_every_value_at_every_position():
    d = dict(delta_cases(576, 12))["nibbles"]
    for row in elements(d):
        for p in range(4):
            assert set(((row >> (4 * p)) & 15).tolist()) == set(range(16))
        assert set(NIBBLES.tolist()) <= set(row.tolist())


@pytest.mark.parametrize("S,n,name", CONTENTS, ids=[f"{S}B-n{n}-{name}" for S, n, name in CONTENTS])
def test_delta_contents(eng, content_plans, S, n, name):
    indices, plan, coef = content_plans[S, n]
    assert_form(plan, M, S, N=n, Q=2 if S == 1600 else 1, nslab=2, rows_per_wave=1, tail=0)
    delta = dict(delta_cases(S, n))[name]
    if name == "zero":
        junk = random_rows(M, S, 7)
        assert np.array_equal(apply_guarded(eng, plan, S, M, junk, delta), junk)
    check_both(eng, plan, K, M, S, indices, delta, coef)


# ---- 3d: a freed plan's address reused ----
# The kernel reads the index array over the scalar path, whose cache a host
# copy does not write through: plan B's array, which the allocator normally
# places where the freed plan A's was, must be read as B's.
@pytest.mark.parametrize("S,n", [(576, 12), (1600, 8)])
def test_freed_plan_address_reused(eng, S, n):
    ia, ib = edge_indices(K, n, 11), edge_indices(K, n, 12)[::-1]
    assert ia != ib
    old, rec_old = stripe(K, M, S)
    da, db = random_rows(n, S, 21), random_rows(n, S, 22)
    v1 = old.copy()
    v1[ia] ^= da
    v2 = v1.copy()
    v2[ib] ^= db
    plan = rs16.UpdatePlan(K, M, ia, engine=eng)
    rec1 = apply_guarded(eng, plan, S, M, rec_old, da)
    plan.close()
    plan = rs16.UpdatePlan(K, M, ib, engine=eng)
    rec2 = apply_guarded(eng, plan, S, M, rec1, db)
    plan.close()
    bad = mismatch(rec1, O.encode(K, M, v1))
    assert not bad, "plan A: " + bad
    bad = mismatch(rec2, O.encode(K, M, v2))
    assert not bad, "plan B: " + bad
    # the one-shot call builds and frees its plans itself: twice in a row
    d_rec = DeviceArray.from_numpy(eng, rec_old)
    d_da, d_db = DeviceArray.from_numpy(eng, da), DeviceArray.from_numpy(eng, db)
    rs16.update_recovery_device(K, M, S, ia, d_da.ptr, d_rec.ptr, engine=eng)
    rs16.update_recovery_device(K, M, S, ib, d_db.ptr, d_rec.ptr, engine=eng)
    bad = mismatch(d_rec.download(shape=(M, S)), O.encode(K, M, v2))
    assert not bad, "update_recovery_device twice: " + bad
