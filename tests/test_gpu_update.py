"""Delta update of recovery shards (rs16_update_plan / rs16_update_device,
rs16_update.hip): a stripe encoded by the oracle
(src/rate/rate_high.rs:44-83, rate_low.rs:44-83), some originals overwritten,
the recovery shards updated on the device from the deltas old ^ new alone --
and compared bit for bit with the oracle's encode of the new stripe.

The geometries take every path of the plan's unit-vector encode (one-pass,
column codec, multi-chunk, three passes, both rates) and every edge of the
kernel: rows narrower than a 512-byte slab, a slab tail (17 blocks), odd row
counts, one row per wave and runs of rows, n = 1 .. 32 -- one and two quads
per lane (rows >= 1 KiB with n <= 8), selectors kept (n <= 16) and extracted
per row (n > 16).
"""
import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


def pick_indices(k, n, seed):
    rng = np.random.default_rng(seed)
    idx = rng.choice(k, n, replace=False).tolist()  # unsorted: delta order = index order
    return [int(i) for i in idx]


def rewrite(old, indices, seed):
    """(new stripe, deltas old ^ new in the order of indices)."""
    rng = np.random.default_rng(seed)
    new = old.copy()
    new[indices] = rng.integers(0, 256, (len(indices), old.shape[1]), dtype=np.uint8)
    return new, old[indices] ^ new[indices]


def check_update(eng, k, m, S, indices, rate="default", seed=1):
    old = generate_original(k, S, seed)
    new, delta = rewrite(old, indices, seed + 100)
    d_rec = DeviceArray.from_numpy(eng, O.encode(k, m, old, rate=rate))
    d_delta = DeviceArray.from_numpy(eng, delta)
    plan = rs16.UpdatePlan(k, m, indices, rate, engine=eng)
    assert len(plan) == len(indices)
    plan.apply(S, d_delta.ptr, d_rec.ptr)
    got = d_rec.download(shape=(m, S))
    plan.close()
    assert np.array_equal(got, O.encode(k, m, new, rate=rate))


# k, m, S, n, rate
GEOMETRIES = [
    (1, 1, 64, 1, "default"),           # smallest stripe
    (3, 5, 128, 2, "default"),
    (5, 3, 64, 5, "low"),
    (100, 300, 192, 7, "default"),
    (300, 100, 1024, 32, "default"),
    (1000, 1000, 1024, 1, "default"),
    (1000, 1000, 1024, 32, "default"),
    (1000, 1025, 1088, 9, "default"),   # 17 blocks give a slab tail; odd row count
    (3000, 1000, 64, 5, "high"),        # multi-chunk
    (513, 1024, 64, 3, "low"),
    (32768, 32768, 64, 3, "default"),   # 65536-row plan
    # two quads per lane (rows >= 1 KiB, n <= 8): the last slab's second column partly / wholly beyond the row
    (300, 100, 1600, 3, "default"),
    (1000, 1025, 1088, 4, "default"),
    (300, 100, 2048, 8, "default"),
    (300, 100, 1024, 9, "default"),     # one quad per lane again
    (1000, 1000, 1024, 17, "default"),  # selectors extracted per row (n > 16)
]


@pytest.mark.parametrize("k,m,S,n,rate", GEOMETRIES, ids=[f"{k}:{m}x{S}-n{n}-{r}" for k, m, S, n, r in GEOMETRIES])
def test_update_equals_reencode(eng, k, m, S, n, rate):
    check_update(eng, k, m, S, pick_indices(k, n, k + n), rate)


def test_pass_codec_plan_edge_indices(eng):
    # 4096:4096 (the plan's encode runs the three HBM passes); first and last originals
    k = m = 4096
    check_update(eng, k, m, 512, [0, 1, k - 2, k - 1])


def test_sub_range(eng):
    """A node holding recovery shards [7, 20) updates only those: the other
    rows and the guard bytes around the buffer keep their contents, and the
    deltas are only read."""
    k, m, S, pos, cnt = 100, 300, 192, 7, 13
    indices = pick_indices(k, 7, 5)
    old = generate_original(k, S, 3)
    new, delta = rewrite(old, indices, 4)
    rec_old, rec_new = O.encode(k, m, old), O.encode(k, m, new)
    guard = np.full(64, 0xEE, np.uint8)
    d_buf = DeviceArray.from_numpy(eng, np.concatenate([guard, rec_old.reshape(-1), guard]))
    d_delta = DeviceArray.from_numpy(eng, delta)
    plan = rs16.UpdatePlan(k, m, indices, engine=eng)
    plan.apply(S, d_delta.ptr, d_buf.offset(64 + pos * S), recovery_pos=pos, recovery_n=cnt)
    got = d_buf.download()
    assert np.array_equal(got[:64], guard) and np.array_equal(got[-64:], guard)
    rows = got[64:-64].reshape(m, S)
    want = rec_old.copy()
    want[pos:pos + cnt] = rec_new[pos:pos + cnt]
    assert np.array_equal(rows, want)
    assert np.array_equal(d_delta.download(shape=delta.shape), delta)
    # the same rows as a buffer of their own (what such a node stores), recovery_n defaulted to the rest
    d_part = DeviceArray.from_numpy(eng, np.concatenate([guard, rec_old[pos:].reshape(-1), guard]))
    plan.apply(S, d_delta.ptr, d_part.offset(64), recovery_pos=pos)
    got = d_part.download()
    assert np.array_equal(got[:64], guard) and np.array_equal(got[-64:], guard)
    assert np.array_equal(got[64:-64].reshape(m - pos, S), rec_new[pos:])


def test_same_plan_twice(eng):
    # two writes to the same shards through one plan = one encode of the final stripe
    k, m, S = 300, 100, 1024
    indices = pick_indices(k, 6, 9)
    v0 = generate_original(k, S, 5)
    v1, d1 = rewrite(v0, indices, 6)
    v2, d2 = rewrite(v1, indices, 7)
    d_rec = DeviceArray.from_numpy(eng, O.encode(k, m, v0))
    d_d1, d_d2 = DeviceArray.from_numpy(eng, d1), DeviceArray.from_numpy(eng, d2)
    plan = rs16.UpdatePlan(k, m, indices, engine=eng)
    plan.apply(S, d_d1.ptr, d_rec.ptr)
    plan.apply(S, d_d2.ptr, d_rec.ptr)
    assert np.array_equal(d_rec.download(shape=(m, S)), O.encode(k, m, v2))


def test_forty_indices_two_plans(eng):
    k, m, S = 1000, 1000, 1024
    indices = pick_indices(k, 40, 13)
    old = generate_original(k, S, 8)
    new, delta = rewrite(old, indices, 9)
    d_rec = DeviceArray.from_numpy(eng, O.encode(k, m, old))
    d_delta = DeviceArray.from_numpy(eng, delta)
    rs16.update_recovery_device(k, m, S, indices, d_delta.ptr, d_rec.ptr, engine=eng)
    assert np.array_equal(d_rec.download(shape=(m, S)), O.encode(k, m, new))


@pytest.mark.parametrize("rate", ["high", "low"])
def test_coefficients_match_oracle_unit_encode(eng, rate):
    k, m = 100, 300
    indices = pick_indices(k, 32, 21)
    unit = np.zeros((k, 64), np.uint8)
    for e, i in enumerate(indices):
        unit[i, e] = 1
    rec = O.encode(k, m, unit, rate=rate)
    want = rec[:, :32].astype(np.uint16) | (rec[:, 32:].astype(np.uint16) << 8)
    plan = rs16.UpdatePlan(k, m, indices, rate, engine=eng)
    got = plan.coefficients()
    assert got.shape == (m, 32) and np.array_equal(got, want)
    assert got.all()


def test_two_engines_on_streams_of_their_own():
    k, m, S = 300, 100, 1024
    old = generate_original(k, S, 15)
    rec_old = O.encode(k, m, old)
    engines = [rs16.Engine(0), rs16.Engine(0)]
    try:
        runs = []
        for j, e in enumerate(engines):
            indices = pick_indices(k, 5 + j, 30 + j)
            new, delta = rewrite(old, indices, 40 + j)
            st = e.create_stream()
            d_rec, d_delta = DeviceArray.from_numpy(e, rec_old), DeviceArray.from_numpy(e, delta)
            plan = rs16.UpdatePlan(k, m, indices, engine=e)
            runs.append((e, st, plan, d_rec, d_delta, new))
        for e, st, plan, d_rec, d_delta, _ in runs:
            plan.apply(S, d_delta.ptr, d_rec.ptr, stream=st)
        for e, st, plan, d_rec, d_delta, new in runs:
            e.synchronize(st)
            assert np.array_equal(d_rec.download(shape=(m, S)), O.encode(k, m, new))
            plan.close()
            e.destroy_stream(st)
    finally:
        for e in engines:
            e.close()


def test_plan_detached_by_engine_close():
    e = rs16.Engine(0)
    plan = rs16.UpdatePlan(100, 300, [1, 2, 3], engine=e)
    d = DeviceArray(e, 300 * 64)
    p = d.ptr
    e.close()
    with pytest.raises(rs16.Error) as x:
        plan.apply(64, p, p)
    assert x.value == rs16.Error("InvalidArgument")
    with pytest.raises(rs16.Error) as x:
        plan.coefficients()
    assert x.value == rs16.Error("InvalidArgument")
    plan.close()  # frees host memory only
    plan.close()


def test_plan_errors(eng):
    E = rs16.Error
    k, m = 100, 300
    for bad in ([], list(range(33))):
        with pytest.raises(E) as x:
            rs16.UpdatePlan(k, m, bad, engine=eng)
        assert x.value == E("InvalidArgument")
    with pytest.raises(E) as x:
        rs16.UpdatePlan(k, m, [0, k], engine=eng)
    assert x.value == E("InvalidOriginalShardIndex", original_count=k, index=k)
    with pytest.raises(E) as x:
        rs16.UpdatePlan(k, m, [4, 9, 4], engine=eng)
    assert x.value == E("DuplicateOriginalShardIndex", index=4)
    with pytest.raises(E) as x:
        rs16.UpdatePlan(4096, 61440, [0], "high", engine=eng)
    assert x.value == E("UnsupportedShardCount", original_count=4096, recovery_count=61440)


def test_apply_errors_and_empty_range(eng):
    E = rs16.Error
    k, m, S = 100, 300, 64
    plan = rs16.UpdatePlan(k, m, [5, 6], engine=eng)
    fill = np.full(m * S, 0x3C, np.uint8)
    d_rec = DeviceArray.from_numpy(eng, fill)
    d_delta = DeviceArray.from_numpy(eng, np.full(2 * S, 0xFF, np.uint8))
    for sb in (0, 100):
        with pytest.raises(E) as x:
            plan.apply(sb, d_delta.ptr, d_rec.ptr)
        assert x.value == E("InvalidShardSize", shard_bytes=sb)
    with pytest.raises(E) as x:
        plan.apply(S, d_delta.ptr, d_rec.ptr, recovery_pos=1, recovery_n=m)  # range end m + 1
    assert x.value == E("InvalidArgument")
    plan.apply(S, d_delta.ptr, d_rec.ptr, recovery_pos=10, recovery_n=0)  # succeeds, writes nothing
    plan.apply(S, d_delta.ptr, d_rec.ptr, recovery_pos=m, recovery_n=0)
    assert np.array_equal(d_rec.download(), fill)
