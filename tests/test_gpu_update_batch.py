"""Delta update of a column window for a batch of stripes in one launch
(rs16_update_device_batch, UpdatePlan.apply_batch, rs16_update_batch.hip,
DESIGN.md 3.22): windows, stripe batches, every kind of kernel instantiation,
the packed form of narrow windows, equality with the single call, the errors
in their order and the decode state.

Every case first asks rs16_host_update_batch_consts (the function the launcher
calls; tests/test_update_batch_consts.py) what is about to run and asserts
the (N, Q, slabs, rows per wave, stripes per wave, rows of the last run) it
was written for.

References, both bit-exact (update_ref.py), as in test_gpu_update_forms.py:
  (a) the oracle's encode of every stripe after the overwrite of the window;
  (b) rec ^ sum_e coef[j, e] . delta_e in numpy from the oracle's exp / log
      tables, on recovery rows of random bytes (no codeword), with coef =
      plan.coefficients() asserted equal to the oracle's unit-vector encode.

The recovery rows lie in ONE buffer  64 guard bytes | stripe 0 | stripe 1 |
... | 64 guard bytes,  stripe i = m whole rows of S bytes (the recovery pitch)
and pad bytes up to the stripe's stride; the deltas in another,  64 guard
bytes | (n windows at the delta pitch, pad bytes) per stripe | 64 guard bytes.
Guards, pad bytes and, for (b), the rows themselves are random bytes.  The
expected buffer is the uploaded one with the window of rows [pos, pos + cnt)
of every stripe replaced; the WHOLE downloaded buffer must equal it, which
covers the guards, the bytes of every row outside the window, the rows outside
the range and the bytes between strides.  The delta buffer must come back as
it went.
"""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from rs16.util import generate_original
from update_batch_ref import batch_consts
from update_ref import edge_indices, table_update, unit_coefficients, update_consts

pytestmark = pytest.mark.gpu

HIGH, LOW = (100, 60, "high"), (60, 100, "low")


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plans(eng):
    """(k, m, rate, n) -> (indices, plan, coef), coef checked against the oracle; shared, closed at the end."""
    made = {}

    def get(k, m, rate, n):
        if (k, m, rate, n) not in made:
            indices = edge_indices(k, n, 100 * m + n)
            plan = rs16.UpdatePlan(k, m, indices, rate, engine=eng)
            coef = plan.coefficients()
            assert np.array_equal(coef, unit_coefficients(k, m, indices, rate)), "plan.coefficients() against the oracle"
            made[k, m, rate, n] = (indices, plan, coef)
        return made[k, m, rate, n]

    yield get
    for _, plan, _ in made.values():
        plan.close()


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@lru_cache(maxsize=None)
def stripe(k, m, S, rate, seed):
    """(old originals, their recovery rows by the oracle), read-only, shared among the cases."""
    old = generate_original(k, S, seed)
    rec = O.encode(k, m, old, rate=rate)
    old.setflags(write=False)
    rec.setflags(write=False)
    return old, rec


def assert_form(n, rows, width, nstripes, Q, nslab, rpw, spw, tail):
    """The kernel and launch shape the case was written for."""
    c = batch_consts(rows, width, n, nstripes)
    got = (c.quads_per_lane, c.nslab, c.rows_per_wave, c.stripes_per_wave, rows % c.rows_per_wave)
    assert got == (Q, nslab, rpw, spw, tail), f"(Q, slabs, rows per wave, stripes per wave, tail) = {got}"
    return c


class Layout:
    """Where the rows and the windows of a case lie in its two buffers."""

    def __init__(self, m, n, S, col, width, nstripes, delta_pitch=None, delta_pad=0, rec_pad=0, pos=0, cnt=None):
        self.m, self.n, self.S, self.col, self.width, self.nstripes = m, n, S, col, width, nstripes
        self.pos, self.cnt = pos, m - pos if cnt is None else cnt
        self.dp = width if delta_pitch is None else delta_pitch
        self.ds, self.rs = n * self.dp + delta_pad, m * S + rec_pad
        assert col + width <= S and col % 64 == 0

    def rows(self, buf, i):
        """Stripe i's (m, S) rows inside the recovery buffer (a view)."""
        return buf[64 + i * self.rs:64 + i * self.rs + self.m * self.S].reshape(self.m, self.S)

    def window(self, buf, i):
        return self.rows(buf, i)[self.pos:self.pos + self.cnt, self.col:self.col + self.width]

    def deltas(self, dbuf, i):
        """Stripe i's (n, width) delta windows inside the delta buffer (a view)."""
        d = dbuf[64 + i * self.ds:64 + i * self.ds + self.n * self.dp].reshape(self.n, self.dp)
        return d[:, :self.width]

    def apply(self, eng, plan, buf, dbuf, stream=None):
        """The call on copies of the two host buffers; asserts that the deltas
        come back unchanged and returns the recovery buffer."""
        d_buf, d_delta = DeviceArray.from_numpy(eng, buf), DeviceArray.from_numpy(eng, dbuf)
        plan.apply_batch(self.width, self.nstripes, d_delta.offset(64), self.dp, self.ds,
                         d_buf.offset(64 + self.pos * self.S + self.col), self.S, self.rs,
                         recovery_pos=self.pos, recovery_n=self.cnt, stream=stream)
        got = d_buf.download()
        assert np.array_equal(d_delta.download(), dbuf), "the deltas were written"
        return got


def mismatch(L, got, want):
    """'' or where two recovery buffers differ, for the assertion's message."""
    if np.array_equal(got, want):
        return ""
    at = np.nonzero(got != want)[0]
    first = int(at[0]) - 64
    i, r, b = first // L.rs, first % L.rs // L.S, first % L.rs % L.S
    return (f"{len(at)} bytes differ, the first at buffer byte {at[0]} (stripe {i}, row {r}, byte {b}; the window is "
            f"rows [{L.pos}, {L.pos + L.cnt}) x bytes [{L.col}, {L.col + L.width})), the last at {at[-1]}")


def check_both(eng, geom, plans, n, L, seed, oracle=True, table=True):
    """References (a) and (b) on one layout."""
    k, m, rate = geom
    indices, plan, coef = plans(k, m, rate, n)
    dbuf = rnd(128 + L.nstripes * L.ds, seed)
    if oracle:
        buf = rnd(128 + L.nstripes * L.rs, seed + 1)
        want = buf.copy()
        for i in range(L.nstripes):
            old, rec_old = stripe(k, m, L.S, rate, 10 + i)
            L.rows(buf, i)[:] = rec_old
            new = old.copy()
            new[indices, L.col:L.col + L.width] ^= L.deltas(dbuf, i)
            rec_new = O.encode(k, m, new, rate=rate)
            L.rows(want, i)[:] = rec_old
            L.rows(want, i)[L.pos:L.pos + L.cnt] = rec_new[L.pos:L.pos + L.cnt]
            # (the re-encode itself changes nothing outside the window)
            outside = np.ones(L.S, bool)
            outside[L.col:L.col + L.width] = False
            assert np.array_equal(rec_new[:, outside], rec_old[:, outside])
        bad = mismatch(L, L.apply(eng, plan, buf, dbuf), want)
        assert not bad, "against the oracle's re-encode: " + bad
    if table:
        buf = rnd(128 + L.nstripes * L.rs, seed + 2)
        want = buf.copy()
        for i in range(L.nstripes):
            L.window(want, i)[:] = table_update(np.ascontiguousarray(L.window(buf, i)), coef[L.pos:L.pos + L.cnt],
                                                np.ascontiguousarray(L.deltas(dbuf, i)))
        bad = mismatch(L, L.apply(eng, plan, buf, dbuf), want)
        assert not bad, "against the table multiply: " + bad


def slabs(width, Q):
    return -(-(width // 8) // (64 * Q))


# ---- windows ----
# Shards of 2048 bytes, n = 4: Q = 2 from 1024 bytes on.  col, width, stripes, delta pitch (None: contiguous), geometry
WINDOWS = [(col, width, ns, dp, geom)
           for col, ns, dp, geom in ((0, 1, "wide", HIGH), (64, 2, None, LOW), (1472, 3, "wide", LOW))
           for width in (64, 576, 1088, 1600) if col + width <= 2048]


@pytest.mark.parametrize("col,width,ns,dp,geom", WINDOWS,
                         ids=[f"{g[2]}-col{c}-w{w}-x{ns}-{'pitched' if dp else 'contiguous'}" for c, w, ns, dp, g in WINDOWS])
def test_window(eng, plans, col, width, ns, dp, geom):
    m, n, S = geom[1], 4, 2048
    L = Layout(m, n, S, col, width, ns, delta_pitch=width + 192 if dp else None, delta_pad=64 if dp else 0, rec_pad=320)
    assert L.dp != S and (dp is None or L.dp != width)
    Q = 2 if width >= 1024 else 1
    spw = 64 // (width // 8) if width <= 128 and ns >= 2 else 1
    assert_form(n, m, width, ns, Q=Q, nslab=slabs(width, Q), rpw=1, spw=spw, tail=0)
    check_both(eng, geom, plans, n, L, seed=col + width)


# ---- batches: stripes, padded strides, sub-ranges ----
# stripes, pos, cnt (None: to the last row), geometry
BATCHES = [(1, 0, None, HIGH), (2, 7, 53, HIGH), (3, 0, 59, LOW), (5, 99, 1, LOW), (5, 31, None, HIGH)]


@pytest.mark.parametrize("ns,pos,cnt,geom", BATCHES, ids=[f"{g[2]}-x{ns}-rows{p}+{c}" for ns, p, c, g in BATCHES])
def test_batch(eng, plans, ns, pos, cnt, geom):
    m, n, S, width = geom[1], 9, 832, 576
    L = Layout(m, n, S, 128, width, ns, delta_pitch=640, delta_pad=192, rec_pad=704, pos=pos, cnt=cnt)
    assert_form(n, L.cnt, width, ns, Q=1, nslab=2, rpw=1, spw=1, tail=0)
    check_both(eng, geom, plans, n, L, seed=ns + pos)


def test_partial_last_run_of_two_rows(eng, plans):
    # 99 rows x 34 slabs x 5 stripes = 16830 waves' worth of rows: runs of two, the last of one row
    k, m, rate = LOW
    n, width, ns = 9, 34 * 512, 5
    L = Layout(m, n, width, 0, width, ns, pos=1, cnt=99)
    c = assert_form(n, 99, width, ns, Q=1, nslab=34, rpw=2, spw=1, tail=1)
    assert c.waves == 50 * 34 * 5
    check_both(eng, LOW, plans, n, L, seed=5, table=False)


def test_partial_last_run_of_32_rows_1000_1000(eng, plans):
    """The cap of 32 rows per wave needs 262144 waves' worth of rows, 128 MiB:
    no smaller shape reaches it.  Reference (b) on random rows, through the
    independence of the column blocks: stripe i's deltas repeat every 67
    blocks (a prime, more blocks than a slab has), so the term XORed into the
    rows is table_update's of 67 blocks, repeated; the rows themselves are
    random and do not repeat."""
    k, m, rate = 1000, 1000, "default"
    n, width, ns, pos, cnt, P = 9, 132 * 512, 2, 1, 999, 67 * 64
    indices, plan, coef = plans(k, m, rate, n)
    L = Layout(m, n, width, 0, width, ns, pos=pos, cnt=cnt)
    c = assert_form(n, cnt, width, ns, Q=1, nslab=132, rpw=32, spw=1, tail=7)
    assert c.waves == 32 * 132 * 2
    dbuf = rnd(128 + ns * L.ds, 3)
    buf = rnd(128 + ns * L.rs, 4)
    want = buf.copy()
    reps = -(-width // P)
    for i in range(ns):
        pattern = rnd(n * P, 50 + i).reshape(n, P)
        L.deltas(dbuf, i)[:] = np.tile(pattern, (1, reps))[:, :width]
        term = table_update(np.zeros((cnt, P), np.uint8), coef[pos:pos + cnt], pattern)
        L.window(want, i)[:] ^= np.tile(term, (1, reps))[:, :width]
    bad = mismatch(L, L.apply(eng, plan, buf, dbuf), want)
    assert not bad, bad


# ---- kernels: the unpacked and the packed instantiations ----
KERNELS = [(n, Q) for n in (1, 4, 8, 9, 16, 17, 32) for Q in (1, 2) if Q == 1 or n <= 8]


@pytest.mark.parametrize("n,Q", KERNELS, ids=[f"n{n}-Q{Q}" for n, Q in KERNELS])
def test_kernels(eng, plans, n, Q):
    # two slabs, the last one partial; three stripes: 60 x 2 x 3 = 360 waves, 90 workgroups
    geom = HIGH if n % 2 else LOW
    m, width = geom[1], 1088 if Q == 2 else 576
    L = Layout(m, n, 1280, 64, width, 3, delta_pitch=1152, rec_pad=128)
    c = assert_form(n, m, width, 3, Q=Q, nslab=2, rpw=1, spw=1, tail=0)
    assert c.waves == m * 6
    check_both(eng, geom, plans, n, L, seed=n + Q)


# width, stripes, n: 8 stripes a wave at 64 bytes (one, a partial, a whole, a whole and one, two and one
# groups), 4 a wave at 128 (a partial, a whole and one, two and one groups)
PACKED = [(64, 2, 1), (64, 7, 4), (64, 8, 8), (64, 9, 9), (64, 17, 16), (64, 9, 17), (64, 9, 32),
          (128, 3, 4), (128, 5, 9), (128, 9, 1)]


@pytest.mark.parametrize("width,ns,n", PACKED, ids=[f"w{w}-x{ns}-n{n}" for w, ns, n in PACKED])
def test_packed(eng, plans, width, ns, n):
    geom = LOW if ns % 2 else HIGH
    m = geom[1]
    spw = 64 // (width // 8)
    L = Layout(m, n, 448, 128, width, ns, delta_pitch=width + 64, delta_pad=128, rec_pad=192, pos=3, cnt=m - 3)
    c = assert_form(n, m - 3, width, ns, Q=1, nslab=1, rpw=1, spw=spw, tail=0)
    assert c.waves == (m - 3) * -(-ns // spw)
    check_both(eng, geom, plans, n, L, seed=width + ns)


# The packed form of 192- and 256-byte windows (two stripes a wave) was measured and not shipped
# (DESIGN.md 3.22): those windows, and 320 bytes, take one stripe a wave.
@pytest.mark.parametrize("width,ns,n", [(192, 3, 4), (256, 2, 9), (256, 5, 1), (320, 5, 4)])
def test_wider_windows_are_not_packed(eng, plans, width, ns, n):
    L = Layout(60, n, 448, 128, width, ns, delta_pitch=384, rec_pad=192)
    assert_form(n, 60, width, ns, Q=1, nslab=1, rpw=1, spw=1, tail=0)
    check_both(eng, HIGH, plans, n, L, seed=width + ns)


# ---- one stripe at full width is the single call ----
@pytest.mark.parametrize("S,n", [(576, 9), (1600, 4), (64, 17)])
def test_one_full_width_stripe_equals_the_single_call(eng, plans, S, n):
    k, m, rate = HIGH
    indices, plan, _ = plans(k, m, rate, n)
    c, one = batch_consts(m, S, n, 1), update_consts(m, S, n)
    assert (c.quads_per_lane, c.nslab, c.rows_per_wave, c.blocks) == tuple(one) and c.stripes_per_wave == 1
    rec, delta = rnd(m * S, 1), rnd(n * S, 2)
    d_a, d_b, d_delta = DeviceArray.from_numpy(eng, rec), DeviceArray.from_numpy(eng, rec), DeviceArray.from_numpy(eng, delta)
    plan.apply(S, d_delta.ptr, d_a.ptr)
    plan.apply_batch(S, 1, d_delta.ptr, S, 0, d_b.ptr, S, 0)  # (one stripe: the strides are not used)
    a, b = d_a.download(), d_b.download()
    assert np.array_equal(a, b) and not np.array_equal(a, rec)


# ---- errors, in their order, with nothing written ----
def c_call(plan_h, width, ns, d_delta, dp, ds, d_rec, rp, rs, pos, cnt):
    err = RS16Error()
    rc = lib().rs16_update_device_batch(plan_h, width, ns, d_delta, dp, ds, d_rec, rp, rs, pos, cnt, None, C.byref(err))
    if rc == 0:
        return "OK"
    e = rs16.Error._from_c(err)
    return (e.kind,) + tuple(e.fields.values())


def test_errors_in_order_and_nothing_written(eng):
    k, m, n, S, width, ns = 100, 60, 3, 256, 128, 2
    plan = rs16.UpdatePlan(k, m, [5, 6, 99], engine=eng)
    dp, ds, rp, rs = 192, 3 * 192, S, m * S
    fill, dfill = rnd(128 + ns * rs, 8), rnd(128 + ns * ds, 9)
    d_rec, d_delta = DeviceArray.from_numpy(eng, fill), DeviceArray.from_numpy(eng, dfill)
    r, d = d_rec.offset(64), d_delta.offset(64)
    INV = ("InvalidArgument",)

    def call(plan_h=plan.h, width=width, ns=ns, d=d, dp=dp, ds=ds, r=r, rp=rp, rs=rs, pos=0, cnt=m):
        return c_call(plan_h, width, ns, d, dp, ds, r, rp, rs, pos, cnt)

    # every later argument wrong as well: the earlier check answers
    assert call(plan_h=None, width=100, pos=m + 1) == INV
    assert call(width=0, pos=m + 1, d=0) == ("InvalidShardSize", 0)
    assert call(width=100, pos=m + 1, d=0) == ("InvalidShardSize", 100)
    assert call(pos=1, cnt=m, d=0) == INV                      # range end m + 1
    assert call(pos=m + 1, cnt=0, ns=0) == INV
    assert call(cnt=0, d=0, r=0, dp=1, rs=1, ns=1 << 20) == "OK"       # nothing to do comes before the layout
    assert call(ns=0, d=0, r=0, dp=1, rs=1, pos=m, cnt=0) == "OK"
    assert call(ns=0, d=1, rp=7) == "OK"
    for bad in (dict(d=0), dict(r=0), dict(d=d + 32), dict(r=r + 16)):
        assert call(**bad) == INV, bad
    for bad in (dict(dp=width - 64), dict(rp=width - 64), dict(dp=dp + 32), dict(rp=rp + 8), dict(dp=0), dict(rp=0)):
        assert call(**bad) == INV, bad
    # strides: whole blocks, and no stripe inside another
    for bad in (dict(ds=ds + 32), dict(rs=rs + 32), dict(rs=(m - 1) * rp + width - 64), dict(rs=0),
                dict(ds=(n - 1) * dp + width - 64), dict(ds=0), dict(pos=10, cnt=20, rs=19 * rp + width - 64)):
        assert call(**bad) == INV, bad
    assert call(ns=65536) == INV
    assert call(ns=1, width=1 << 32, dp=1 << 32, rp=1 << 32) == INV
    assert call(ns=1, dp=1 << 32) == INV and call(ns=1, rp=1 << 32) == INV
    assert np.array_equal(d_rec.download(), fill) and np.array_equal(d_delta.download(), dfill), "an error wrote"
    # the tightest layout that is allowed: stripes that end where the next one's window begins
    assert call(pos=10, cnt=20, rs=19 * rp + width, ds=(n - 1) * dp + width) == "OK"
    # one stripe has no strides
    assert call(ns=1, ds=1, rs=1) == "OK"
    eng.synchronize()
    # the Python method raises the same errors
    with pytest.raises(rs16.Error) as x:
        plan.apply_batch(100, ns, d, dp, ds, r, rp, rs)
    assert x.value == rs16.Error("InvalidShardSize", shard_bytes=100)
    with pytest.raises(rs16.Error) as x:
        plan.apply_batch(width, ns, d, dp, ds, r, rp, rs - 64 * m)
    assert x.value == rs16.Error("InvalidArgument")
    plan.close()


def test_nothing_to_do_leaves_the_guards(eng):
    k, m, n, S = 100, 60, 2, 128
    plan = rs16.UpdatePlan(k, m, [0, 99], engine=eng)
    L = Layout(m, n, S, 0, S, 2)
    buf, dbuf = rnd(128 + 2 * L.rs, 1), rnd(128 + 2 * L.ds, 2)
    d_buf, d_delta = DeviceArray.from_numpy(eng, buf), DeviceArray.from_numpy(eng, dbuf)
    plan.apply_batch(S, 0, d_delta.offset(64), L.dp, L.ds, d_buf.offset(64), S, L.rs)
    plan.apply_batch(S, 2, d_delta.offset(64), L.dp, L.ds, d_buf.offset(64), S, L.rs, recovery_pos=5, recovery_n=0)
    plan.apply_batch(S, 2, d_delta.offset(64), L.dp, L.ds, d_buf.offset(64), S, L.rs, recovery_pos=m)
    assert np.array_equal(d_buf.download(), buf) and np.array_equal(d_delta.download(), dbuf)
    plan.close()


def test_plan_detached_by_engine_close():
    e = rs16.Engine(0)
    plan = rs16.UpdatePlan(100, 60, [1, 2, 3], engine=e)
    d = DeviceArray(e, 2 * 60 * 64)
    p = d.ptr
    e.close()
    with pytest.raises(rs16.Error) as x:
        plan.apply_batch(64, 2, p, 64, 192, p, 64, 60 * 64)
    assert x.value == rs16.Error("InvalidArgument")
    assert c_call(plan.h, 100, 2, p, 64, 192, p, 64, 60 * 64, 0, 60) == ("InvalidArgument",)  # before the width
    plan.close()  # frees host memory only
    plan.close()


# ---- the decode state ----
def test_update_batch_keeps_decode_state(eng, plans):
    """An update is not a decode: a pending rs16_decode_prepare survives the
    call and rs16_decode_check still reports the last decode."""
    k, m, sb = 100, 100, 192
    original, recovery = stripe(k, m, sb, "default", 3)

    def update_ok():
        L = Layout(60, 4, 448, 128, 64, 9, delta_pitch=128, rec_pad=192)
        check_both(eng, HIGH, plans, 4, L, seed=77, oracle=False)

    of = np.ones(k, np.uint8)
    of[[1, 50, 99]] = 0
    held = original.copy()
    held[of == 0] = 0xA5
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, recovery)
    d_fo, d_fr = DeviceArray.from_numpy(eng, of), DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    # an update between the prepare and the prepared decode
    rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, k - 3, m, engine=eng)
    update_ok()
    rs16.decode_device_prepared(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_o.download(shape=(k, sb)), original)
    # a decode given a wrong count, then an update: rs16_decode_check still reports that decode
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 2, m, engine=eng)
    update_ok()
    err = RS16Error()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) != 0
    assert (err.v0, err.v1) == (k - 3, m)
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 3, m, engine=eng)
    update_ok()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) == 0
