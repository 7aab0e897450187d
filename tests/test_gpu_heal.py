"""rs16_locate_device_batch, rs16_heal_device and rs16_heal_device_batch
(include/rs16.h "Heal"): the locate for batches of stripes, and the fix applied
on the device.

Expected values never come from the library: status, shard and fix of every
stripe are those of the brute-force locator of tests/test_locate_matrix.py, and
the expected healed stripe is the stored stripe with that reference's fix XORed
in on the host.  In the batch of 2500 tiny stripes only the four corrupted ones
go through the reference; the others are the oracle's encode, CLEAN by
construction.

Every buffer is guarded as in tests/test_gpu_locate.py: outputs pre-filled 0xA5
with 0xFF before, behind and between the strides (status and fix at odd
addresses), shard arrays with 0x5A between and behind the stripes, both read
back whole after every call.  All strides of the batch calls are larger than
their arrays.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from test_gpu_locate import patterns, stripe
from test_locate_matrix import CLEAN, NO_SHARD, ORIGINAL, RECOVERY, UNLOCATABLE, ref_locate

pytestmark = pytest.mark.gpu

GUARD = 64
BOTH = rs16.HEAL_ORIGINAL | rs16.HEAL_RECOVERY


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def plan_for(eng, k, m, rate="default"):
    return rs16.LocatePlan(k, m, rate, engine=eng)


@functools.lru_cache(maxsize=None)
def case(k, m, sb, name, rate="default"):
    """(stored originals, stored recovery, reference status, shard, fix) of one
    pattern of tests/test_gpu_locate.py's, computed once, read-only."""
    original, recovery = stripe(k, m, sb, rate)
    o, r = patterns(k, m, sb, original, recovery)[name]
    out = (o, r) + ref_locate(k, m, o, r, rate)
    for a in out:
        a.setflags(write=False)
    return out


class Strided:
    """n device output ranges of `used` bytes, `stride` bytes apart from byte
    `off` of a buffer: 0xA5 in the ranges, 0xFF before, between and behind."""

    def __init__(self, eng, n, used, stride, off, pad=8):
        self.n, self.used, self.stride, self.off = n, used, stride, off
        self.host = np.full(off + (n - 1) * stride + used + pad, 0xFF, np.uint8)
        self.inside = np.zeros(self.host.size, bool)
        for i in range(n):
            self.inside[off + i * stride:off + i * stride + used] = True
        self.host[self.inside] = 0xA5
        self.d = DeviceArray.from_numpy(eng, self.host)
        self.ptr = self.d.ptr + off

    def read(self, dtype=np.uint8):
        got = self.d.download()
        assert (got[~self.inside] == 0xFF).all(), "bytes outside the used ranges written"
        return got[self.inside].view(dtype).reshape(self.n, -1)

    def untouched(self):
        return np.array_equal(self.d.download(), self.host)


class Stored:
    """The stripes of a batch on the device: stripe i's k x sb originals at i
    o_stride, its m x sb recovery at i r_stride, 0x5A between and behind."""

    def __init__(self, eng, k, m, sb, stripes, o_pad=64, r_pad=128):
        self.k, self.m, self.sb, self.n = k, m, sb, len(stripes)
        self.o_stride, self.r_stride = k * sb + o_pad, m * sb + r_pad
        self.host_o = np.full(self.n * self.o_stride + GUARD, 0x5A, np.uint8)
        self.host_r = np.full(self.n * self.r_stride + GUARD, 0x5A, np.uint8)
        for i, (o, r) in enumerate(stripes):
            self.host_o[i * self.o_stride:i * self.o_stride + k * sb] = o.reshape(-1)
            self.host_r[i * self.r_stride:i * self.r_stride + m * sb] = r.reshape(-1)
        self.d_o, self.d_r = DeviceArray.from_numpy(eng, self.host_o), DeviceArray.from_numpy(eng, self.host_r)

    def unchanged(self):
        assert np.array_equal(self.d_o.download(), self.host_o), "originals (or their guard) written"
        assert np.array_equal(self.d_r.download(), self.host_r), "recovery (or its guard) written"

    def expect(self, o_exp, r_exp):
        """Both arrays, guards included, equal the host's with the stripes replaced by o_exp / r_exp."""
        want_o, want_r = self.host_o.copy(), self.host_r.copy()
        for i in range(self.n):
            want_o[i * self.o_stride:i * self.o_stride + self.k * self.sb] = o_exp[i].reshape(-1)
            want_r[i * self.r_stride:i * self.r_stride + self.m * self.sb] = r_exp[i].reshape(-1)
        assert np.array_equal(self.d_o.download(), want_o), "originals differ from the host-healed stripes"
        assert np.array_equal(self.d_r.download(), want_r), "recovery differs from the host-healed stripes"


def locate_batch(eng, plan, k, m, sb, stripes, fix=True):
    """One rs16_locate_device_batch call: (status [n, B], shard [n, B], fix [n, B, 64] or None)."""
    n, B = len(stripes), sb // 64
    d = Stored(eng, k, m, sb, stripes)
    st = Strided(eng, n, B, B + 3, off=1)
    sh = Strided(eng, n, 4 * B, 4 * (B + 2), off=4)
    fx = Strided(eng, n, 64 * B, 64 * B + 7, off=3) if fix else None
    plan.locate_batch(sb, n, d.d_o, d.o_stride, d.d_r, d.r_stride, st.ptr, B + 3, sh.ptr, B + 2,
                      fx.ptr if fix else None, 64 * B + 7 if fix else 0)
    eng.synchronize()
    d.unchanged()
    return st.read(), sh.read(np.uint32), fx.read().reshape(n, B, 64) if fix else None


def locate_single(eng, plan, sb, o, r):
    B = sb // 64
    d_o, d_r = DeviceArray.from_numpy(eng, o), DeviceArray.from_numpy(eng, r)
    st, sh, fx = Strided(eng, 1, B, B, off=1), Strided(eng, 1, 4 * B, 4 * B, off=4), Strided(eng, 1, 64 * B, 64 * B, off=3)
    plan.locate(sb, d_o, d_r, st.ptr, sh.ptr, fx.ptr)
    return st.read()[0], sh.read(np.uint32)[0], fx.read().reshape(B, 64)


def heal_batch(eng, plan, k, m, sb, stripes, mask=BOTH, outputs=True, single=False):
    """One heal call on guarded buffers: (the stored batch, status, shard, counts [n, 4])."""
    n, B = len(stripes), sb // 64
    d = Stored(eng, k, m, sb, stripes)
    st = Strided(eng, n, B, B + 3, off=1) if outputs else None
    sh = Strided(eng, n, 4 * B, 4 * (B + 2), off=4) if outputs else None
    ct = Strided(eng, n, 16, 20, off=4)
    if single:
        assert n == 1
        plan.heal(sb, d.d_o, d.d_r, ct.ptr, mask, st.ptr if outputs else None, sh.ptr if outputs else None)
    else:
        plan.heal_batch(sb, n, d.d_o, d.o_stride, d.d_r, d.r_stride, ct.ptr, 5, mask,
                        st.ptr if outputs else None, B + 3, sh.ptr if outputs else None, B + 2)
    eng.synchronize()
    return d, st.read() if outputs else None, sh.read(np.uint32) if outputs else None, ct.read(np.uint32)


def reference(cases):
    """The stripes (stored originals, stored recovery) and the reference's status / shard / fix, stacked."""
    return ([(c[0], c[1]) for c in cases], np.stack([c[2] for c in cases]), np.stack([c[3] for c in cases]),
            np.stack([c[4] for c in cases]))


def host_healed(stripes, st, sh, fx, mask):
    """The stored stripes with the reference's fix XORed in by the heal's rules."""
    o_exp, r_exp = [o.copy() for o, _ in stripes], [r.copy() for _, r in stripes]
    for i in range(len(stripes)):
        for c in np.flatnonzero(st[i]):
            if st[i, c] == ORIGINAL and mask & rs16.HEAL_ORIGINAL:
                o_exp[i][sh[i, c], 64 * c:64 * c + 64] ^= fx[i, c]
            if st[i, c] == RECOVERY and mask & rs16.HEAL_RECOVERY:
                r_exp[i][sh[i, c], 64 * c:64 * c + 64] ^= fx[i, c]
    return o_exp, r_exp


def histogram(st):
    return np.stack([np.bincount(row, minlength=4)[:4] for row in st]).astype(np.uint32)


MIXED = ("clean", "o_random_shard", "r_last", "two_o_one_block", "o_block0_r_last_block")
# k, m, sb, rate, the pattern of each stripe
BATCH_MIXED = [(5, 3, 192, "default", MIXED), (3, 5, 192, "low", MIXED)]
#   1000:1000 x 1088: the column codec, the batched encode, 17 blocks; 3000:1000 and 300:2000:
#   multi-chunk, encoded stripe by stripe; 5:3 x 2112: two scan workgroups side by side;
#   3:5 x 65600: one copy of the pairs; 300:2: m = 2
BATCH_FORMS = [(1000, 1000, 1088, "default", ("o_random_shard", "r_last", "clean")),
               (3000, 1000, 64, "default", ("o_random_shard", "r_last")),
               (300, 2000, 64, "default", ("r_last", "o_random_shard")),
               (5, 3, 2112, "default", ("o_random_shard", "r_last")),
               (3, 5, 65600, "default", ("clean", "o_random_shard")),
               (300, 2, 192, "default", ("r_last", "o_random_shard"))]


def batch_cases(k, m, sb, rate, names):
    return reference([case(k, m, sb, name, rate) for name in names])


@pytest.mark.parametrize("k,m,sb,rate,names", BATCH_MIXED + BATCH_FORMS)
def test_locate_batch(eng, k, m, sb, rate, names):
    stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, rate, names)
    plan = plan_for(eng, k, m, rate)
    st, sh, fx = locate_batch(eng, plan, k, m, sb, stripes)
    assert np.array_equal(st, want_st), (st, want_st)
    assert np.array_equal(sh, want_sh), (sh, want_sh)
    assert np.array_equal(fx, want_fx), np.argwhere((fx != want_fx).any(axis=2))
    if names is MIXED:
        assert set(want_st.reshape(-1).tolist()) == {CLEAN, ORIGINAL, RECOVERY, UNLOCATABLE}
        # the single call, stripe by stripe
        for i, (o, r) in enumerate(stripes):
            one = locate_single(eng, plan, sb, o, r)
            for g, w in zip(one, (st[i], sh[i], fx[i])):
                assert np.array_equal(g, w), (i, g, w)
        # and without the fix
        st, sh, none = locate_batch(eng, plan, k, m, sb, stripes, fix=False)
        assert none is None and np.array_equal(st, want_st) and np.array_equal(sh, want_sh)


@functools.lru_cache(maxsize=None)
def many_small():
    """2:3 x 64 B x 2500: the oracle's encode of random originals; stripes 0, 1,
    1249 and 2499 corrupted: one original bit, one recovery bit, two originals at
    one element, one original bit."""
    k, m, sb, n = 2, 3, 64, 2500
    rng = np.random.default_rng(2500)
    clean_o = rng.integers(0, 256, (n, k, sb), dtype=np.uint8)
    clean_r = np.stack([O.encode(k, m, clean_o[i]) for i in range(n)])
    o, r = clean_o.copy(), clean_r.copy()
    o[0, 1, 7] ^= 0x10
    r[1, 2, 40] ^= 0x01
    o[1249, 0, 5] ^= 0x01
    o[1249, 1, 5] ^= 0x02
    o[2499, 0, 63] ^= 0x80
    st = np.zeros((n, 1), np.uint8)
    sh = np.full((n, 1), NO_SHARD, np.uint32)
    fx = np.zeros((n, 1, 64), np.uint8)
    for i in (0, 1, 1249, 2499):
        st[i], sh[i], fx[i] = ref_locate(k, m, o[i], r[i])
    for a in (clean_o, clean_r, o, r, st, sh, fx):
        a.setflags(write=False)
    return clean_o, clean_r, o, r, st, sh, fx


def test_locate_many_stripes(eng):
    """More stripes than the scan's workgroup target: one row chunk each."""
    k, m, sb, n = 2, 3, 64, 2500
    assert n > 2048 and rs16.locate_scan_shape(sb, m, n)[3] == 1
    _, _, o, r, want_st, want_sh, want_fx = many_small()
    assert want_st[[0, 1, 1249, 2499], 0].tolist() == [ORIGINAL, RECOVERY, UNLOCATABLE, ORIGINAL]
    st, sh, fx = locate_batch(eng, plan_for(eng, k, m), k, m, sb, list(zip(o, r)))
    assert np.array_equal(st, want_st), np.flatnonzero((st != want_st).any(axis=1))
    assert np.array_equal(sh, want_sh), np.flatnonzero((sh != want_sh).any(axis=1))
    assert np.array_equal(fx, want_fx), np.flatnonzero((fx != want_fx).any(axis=(1, 2)))


def check_healed(eng, d, stripes, clean, want_st, want_sh, want_fx, st, sh, counts, mask, rate):
    """What a heal must leave: the host-healed stripes and guards, the
    reference's status / shard as found before the fix, and the histogram."""
    o_exp, r_exp = host_healed(stripes, want_st, want_sh, want_fx, mask)
    d.expect(o_exp, r_exp)
    if st is not None:
        assert np.array_equal(st, want_st) and np.array_equal(sh, want_sh)
    assert np.array_equal(counts, histogram(want_st)), (counts, histogram(want_st))
    if mask != BOTH:
        return
    k, m, sb, n = d.k, d.m, d.sb, d.n
    for i in range(n):
        for c in range(sb // 64):
            cols = slice(64 * c, 64 * c + 64)
            if want_st[i, c] == UNLOCATABLE:  # keeps its stored bytes exactly
                assert np.array_equal(o_exp[i][:, cols], stripes[i][0][:, cols]), (i, c)
                assert np.array_equal(r_exp[i][:, cols], stripes[i][1][:, cols]), (i, c)
            else:  # back to the clean bytes
                assert np.array_equal(o_exp[i][:, cols], clean[i][0][:, cols]), (i, c)
                assert np.array_equal(r_exp[i][:, cols], clean[i][1][:, cols]), (i, c)
    if rate == "default":
        # the scrub afterwards flags exactly the stripes with a block left UNLOCATABLE
        d_rows = DeviceArray(eng, n * m)
        rs16.verify_device_batch(k, m, sb, n, d.d_o, d.o_stride, d.d_r, d.r_stride, d_rows, m, engine=eng)
        flagged = d_rows.download(shape=(n, m)).any(axis=1)
        assert np.array_equal(flagged, (want_st == UNLOCATABLE).any(axis=1)), np.flatnonzero(flagged)


@pytest.mark.parametrize("k,m,sb,rate,names", BATCH_MIXED + BATCH_FORMS)
def test_heal_batch(eng, k, m, sb, rate, names):
    stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, rate, names)
    clean = [stripe(k, m, sb, rate)] * len(stripes)
    d, st, sh, counts = heal_batch(eng, plan_for(eng, k, m, rate), k, m, sb, stripes)
    check_healed(eng, d, stripes, clean, want_st, want_sh, want_fx, st, sh, counts, BOTH, rate)


def test_heal_many_stripes(eng):
    k, m, sb = 2, 3, 64
    clean_o, clean_r, o, r, want_st, want_sh, want_fx = many_small()
    stripes = list(zip(o, r))
    d, st, sh, counts = heal_batch(eng, plan_for(eng, k, m), k, m, sb, stripes)
    check_healed(eng, d, stripes, list(zip(clean_o, clean_r)), want_st, want_sh, want_fx, st, sh, counts, BOTH,
                 "default")


@pytest.mark.parametrize("mask", [rs16.HEAL_ORIGINAL, rs16.HEAL_RECOVERY])
def test_heal_one_kind(eng, mask):
    """The array outside the mask stays bit-identical; status, shard and counts do not change."""
    k, m, sb, rate, names = BATCH_MIXED[0]
    stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, rate, names)
    assert (want_st == ORIGINAL).any() and (want_st == RECOVERY).any()
    d, st, sh, counts = heal_batch(eng, plan_for(eng, k, m), k, m, sb, stripes, mask)
    check_healed(eng, d, stripes, None, want_st, want_sh, want_fx, st, sh, counts, mask, rate)
    if mask == rs16.HEAL_ORIGINAL:
        assert np.array_equal(d.d_r.download(), d.host_r)
        assert not np.array_equal(d.d_o.download(), d.host_o)
    else:
        assert np.array_equal(d.d_o.download(), d.host_o)
        assert not np.array_equal(d.d_r.download(), d.host_r)


def test_heal_without_status_and_shard(eng):
    k, m, sb, rate, names = BATCH_MIXED[0]
    stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, rate, names)
    clean = [stripe(k, m, sb)] * len(stripes)
    d, st, sh, counts = heal_batch(eng, plan_for(eng, k, m), k, m, sb, stripes, outputs=False)
    check_healed(eng, d, stripes, clean, want_st, want_sh, want_fx, None, None, counts, BOTH, rate)


@pytest.mark.parametrize("k,m,sb", [(5, 3, 192), (1000, 1000, 1088)])
def test_heal_single(eng, k, m, sb):
    plan = plan_for(eng, k, m)
    clean = [stripe(k, m, sb)]
    for name, outputs in (("o_block0_r_last_block", True), ("two_o_one_block", True), ("o_random_shard", False)):
        stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, "default", (name,))
        d, st, sh, counts = heal_batch(eng, plan, k, m, sb, stripes, outputs=outputs, single=True)
        check_healed(eng, d, stripes, clean, want_st, want_sh, want_fx, st, sh, counts, BOTH, "default")
    # a clean stripe: nothing written
    B = sb // 64
    d, st, sh, counts = heal_batch(eng, plan, k, m, sb, clean, single=True)
    d.unchanged()
    assert not st.any() and (sh == NO_SHARD).all()
    assert counts.tolist() == [[B, 0, 0, 0]]


def test_host_level_heal(eng):
    k, m, sb = 100, 7, 192
    original, recovery = stripe(k, m, sb)
    o, r, want_st, want_sh, want_fx = case(k, m, sb, "o_block0_r_last_block")
    ho, hr, st, sh, counts = rs16.heal(k, m, list(o), list(r), engine=eng)
    assert np.array_equal(ho, original) and np.array_equal(hr, recovery)
    assert st.dtype == np.uint8 and sh.dtype == np.uint32 and counts.dtype == np.uint32
    assert np.array_equal(st, want_st) and np.array_equal(sh, want_sh)
    assert np.array_equal(counts, histogram(want_st[None])[0])
    ho, hr, st, sh, counts = rs16.heal(k, m, o, r, rs16.HEAL_RECOVERY, engine=eng)
    o_exp, r_exp = host_healed([(o, r)], want_st[None], want_sh[None], want_fx[None], rs16.HEAL_RECOVERY)
    assert np.array_equal(ho, o_exp[0]) and np.array_equal(hr, r_exp[0]) and np.array_equal(ho, o)


def test_engine_state_across_sizes():
    """The engine's error array and pairs are zero between calls whatever the
    next call's stripes: single, batch, single, smaller batch, heal batch, and a
    second geometry, every answer right."""
    e = rs16.Engine(0)
    try:
        k, m, sb = 100, 7, 192
        plan = rs16.LocatePlan(k, m, engine=e)
        names = ("o_random_shard", "o_block0_r_last_block", "clean", "two_o_one_block", "r_last")
        stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, "default", names)
        original, recovery = stripe(k, m, sb)

        def single(o, r, want):
            for g, w in zip(locate_single(e, plan, sb, o, r), want):
                assert np.array_equal(g, w), (g, w)

        def batch(idx):
            got = locate_batch(e, plan, k, m, sb, [stripes[i] for i in idx])
            for g, w in zip(got, (want_st, want_sh, want_fx)):
                assert np.array_equal(g, w[list(idx)]), (idx, g)

        single(*stripes[0], (want_st[0], want_sh[0], want_fx[0]))
        batch(range(5))
        B = sb // 64
        single(original, recovery, (np.zeros(B, np.uint8), np.full(B, NO_SHARD, np.uint32), np.zeros((B, 64), np.uint8)))
        batch((3, 1))
        d, st, sh, counts = heal_batch(e, plan, k, m, sb, stripes)
        check_healed(e, d, stripes, [(original, recovery)] * 5, want_st, want_sh, want_fx, st, sh, counts, BOTH,
                     "default")
        k2, m2, sb2 = 40, 70, 64
        plan2 = rs16.LocatePlan(k2, m2, engine=e)
        st, sh, fx = locate_single(e, plan2, sb2, *stripe(k2, m2, sb2))
        assert st.tolist() == [CLEAN] and sh.tolist() == [NO_SHARD] and not fx.any()
        plan.close()
        plan2.close()
    finally:
        e.close()


def kind(rc, err):
    return rs16.Error._from_c(err).kind if rc else None


def c_locate_batch(plan_h, sb, n, o, os, r, rs, st, sts, sh, shs, fx=None, fxs=0):
    err = RS16Error()
    return kind(lib().rs16_locate_device_batch(plan_h, sb, n, o, os, r, rs, st, sts, sh, shs, fx, fxs, None,
                                               C.byref(err)), err)


def c_heal(plan_h, sb, o, r, mask, st, sh, ct):
    err = RS16Error()
    return kind(lib().rs16_heal_device(plan_h, sb, o, r, mask, st, sh, ct, None, C.byref(err)), err)


def c_heal_batch(plan_h, sb, n, o, os, r, rs, mask, st, sts, sh, shs, ct, cts):
    err = RS16Error()
    return kind(lib().rs16_heal_device_batch(plan_h, sb, n, o, os, r, rs, mask, st, sts, sh, shs, ct, cts, None,
                                             C.byref(err)), err)


def test_errors_in_order(eng):
    k, m, sb, n = 100, 7, 64, 3
    plan = plan_for(eng, k, m)
    os_, rs_ = k * sb, m * sb
    d = DeviceArray(eng, n * k * sb + 128)
    f = DeviceArray(eng, 4096)
    st, sh, fx, ct = f.ptr, f.ptr + 64, f.ptr + 1024, f.ptr + 256
    # no plan: whatever else is wrong
    assert c_locate_batch(None, 100, n, None, 0, None, 0, None, 0, None, 0) == "InvalidArgument"
    assert c_heal(None, 100, None, None, 0, None, None, None) == "InvalidArgument"
    assert c_heal_batch(None, 100, n, None, 0, None, 0, 0, None, 0, None, 0, None, 0) == "InvalidArgument"
    # then the shard size
    for bad in (0, 100, 2**32):
        assert c_locate_batch(plan.h, bad, n, None, 0, d.ptr + 1, 0, None, 0, None, 0) == "InvalidShardSize"
        assert c_heal(plan.h, bad, None, d.ptr + 1, 0, None, None, None) == "InvalidShardSize"
        assert c_heal_batch(plan.h, bad, n, None, 0, None, 0, 0, None, 0, None, 0, None, 0) == "InvalidShardSize"
    # then the locate's arguments
    for o, r in ((None, d.ptr), (d.ptr, None), (d.ptr + 32, d.ptr), (d.ptr, d.ptr + 16)):
        assert c_locate_batch(plan.h, sb, n, o, os_, r, rs_, st, 1, sh, 1, fx, 64) == "InvalidArgument"
        assert c_heal(plan.h, sb, o, r, BOTH, st, sh, ct) == "InvalidArgument"
        assert c_heal_batch(plan.h, sb, n, o, os_, r, rs_, BOTH, st, 1, sh, 1, ct, 4) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, None, 1, sh, 1) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, st, 1, None, 1) == "InvalidArgument"
    # the heal's mask, then its counts
    for mask in (0, 4, 7, -1):
        assert c_heal(plan.h, sb, d.ptr, d.ptr, mask, st, sh, ct) == "InvalidArgument"
        assert c_heal_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, mask, st, 1, sh, 1, ct, 4) == "InvalidArgument"
    assert c_heal(plan.h, sb, d.ptr, d.ptr, BOTH, st, sh, None) == "InvalidArgument"
    assert c_heal_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, BOTH, st, 1, sh, 1, None, 4) == "InvalidArgument"
    # the batch forms: the shard strides, the output strides, the stripe count
    for bo, br in ((os_ - 64, rs_), (os_, rs_ - 64), (os_ + 32, rs_), (os_, rs_ + 16)):
        assert c_locate_batch(plan.h, sb, n, d.ptr, bo, d.ptr, br, st, 1, sh, 1, fx, 64) == "InvalidArgument"
        assert c_heal_batch(plan.h, sb, n, d.ptr, bo, d.ptr, br, BOTH, st, 1, sh, 1, ct, 4) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, st, 0, sh, 1, fx, 64) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, st, 1, sh, 0, fx, 64) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, st, 1, sh, 1, fx, 63) == "InvalidArgument"
    assert c_heal_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, BOTH, st, 0, sh, 1, ct, 4) == "InvalidArgument"
    assert c_heal_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, BOTH, st, 1, sh, 0, ct, 4) == "InvalidArgument"
    assert c_heal_batch(plan.h, sb, n, d.ptr, os_, d.ptr, rs_, BOTH, st, 1, sh, 1, ct, 3) == "InvalidArgument"
    assert c_locate_batch(plan.h, sb, 65536, d.ptr, os_, d.ptr, rs_, st, 1, sh, 1, fx, 64) == "InvalidArgument"
    assert c_heal_batch(plan.h, sb, 65536, d.ptr, os_, d.ptr, rs_, BOTH, st, 1, sh, 1, ct, 4) == "InvalidArgument"
    # no stripes: nothing launched, nothing written (after the checks: a bad stride still fails)
    out = Strided(eng, 1, 2048, 2048, off=1)
    p = out.ptr
    assert c_locate_batch(plan.h, sb, 0, d.ptr, os_, d.ptr, rs_, p, 1, p + 63, 1, p + 1024, 64) is None
    assert c_heal_batch(plan.h, sb, 0, d.ptr, os_, d.ptr, rs_, BOTH, p, 1, p + 63, 1, p + 255, 4) is None
    assert c_heal_batch(plan.h, sb, 0, d.ptr, os_, d.ptr, rs_, BOTH, p, 1, p + 63, 1, p + 255, 3) == "InvalidArgument"
    eng.synchronize()
    assert out.untouched()


def test_detached_plan_fails_after_engine_free():
    e2 = rs16.Engine(0)
    plan = rs16.LocatePlan(5, 3, engine=e2)
    d = DeviceArray.from_numpy(e2, np.zeros(2 * 5 * 64, np.uint8))
    f = DeviceArray(e2, 1024)
    o, st, sh, fx, ct = d.ptr, f.ptr, f.ptr + 64, f.ptr + 128, f.ptr + 512
    assert c_locate_batch(plan.h, 64, 2, o, 320, o, 192, st, 1, sh, 1, fx, 64) is None
    assert c_heal(plan.h, 64, o, o, BOTH, st, sh, ct) is None
    assert c_heal_batch(plan.h, 64, 2, o, 320, o, 192, BOTH, st, 1, sh, 1, ct, 4) is None
    e2.synchronize()
    e2.close()
    assert c_locate_batch(plan.h, 64, 2, o, 320, o, 192, st, 1, sh, 1, fx, 64) == "InvalidArgument"
    assert c_heal(plan.h, 64, o, o, BOTH, st, sh, ct) == "InvalidArgument"
    assert c_heal_batch(plan.h, 64, 2, o, 320, o, 192, BOTH, st, 1, sh, 1, ct, 4) == "InvalidArgument"
    with pytest.raises(rs16.Error):
        plan.heal_batch(64, 2, o, 320, o, 192, ct)
    plan.close()
    plan.close()


def test_heal_keeps_decode_state(eng):
    """Like the locate, a heal is not a decode: a pending rs16_decode_prepare
    survives it and rs16_decode_check still reports the last decode."""
    k, m, sb = 100, 100, 192
    original, recovery = stripe(k, m, sb)
    plan = plan_for(eng, k, m)
    names = ("o_block0_r_last_block", "clean")
    stripes, want_st, want_sh, want_fx = batch_cases(k, m, sb, "default", names)

    def heal_ok():
        d, st, sh, counts = heal_batch(eng, plan, k, m, sb, stripes)
        check_healed(eng, d, stripes, [(original, recovery)] * 2, want_st, want_sh, want_fx, st, sh, counts, BOTH,
                     "no scrub")

    of = np.ones(k, np.uint8)
    of[[1, 50, 99]] = 0
    held = original.copy()
    held[of == 0] = 0xA5
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, recovery)
    d_fo, d_fr = DeviceArray.from_numpy(eng, of), DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    # a heal between the prepare and the prepared decode
    rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, k - 3, m, engine=eng)
    heal_ok()
    rs16.decode_device_prepared(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_o.download(shape=(k, sb)), original)
    # a decode given a wrong count, then a heal: rs16_decode_check still reports that decode
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 2, m, engine=eng)
    heal_ok()
    err = RS16Error()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) != 0
    assert (err.v0, err.v1) == (k - 3, m)
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 3, m, engine=eng)
    heal_ok()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) == 0
