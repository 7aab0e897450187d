"""rs16_locate_plan / rs16_locate_device (include/rs16.h "Locate"): which one
shard of each 64-byte column block is corrupt, and the bytes that fix it.

Expected values never come from the library: status, shard and fix of every
case are those of the brute-force locator of tests/test_locate_matrix.py (the
oracle's encode, M from the oracle's unit-vector encodes, every single-shard
explanation checked against all recovery rows), and at 32768:32768 those of the
construction (one flipped bit of one shard; the stored recovery is the
oracle's encode).  Every call writes status, shard and fix into guarded buffers
pre-filled with 0xA5 (status and fix at odd addresses) and reads both shard
arrays back, guard included.

Shapes: 5:3 and 3:5 (both rates, one pass), 100:7, 40:70, 300:2 (m = 2),
1000:1000 x 1088 (the column codec's encode; 17 blocks, not a multiple of the
scan's lanes), 3000:1000 and 300:2000 (multi-chunk, both rates), 5:3 x 2112 and
3:5 x 65600 (the scan's other launch shapes, see SHAPES), 32768:32768 (k at its
maximum: 64 plan chunks, shard indices that need 15 bits).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from test_locate_matrix import CLEAN, NO_SHARD, ORIGINAL, RECOVERY, UNLOCATABLE, matrix, ref_locate

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def plan_for(eng, k, m, rate="default"):
    return rs16.LocatePlan(k, m, rate, engine=eng)


@functools.lru_cache(maxsize=None)
def stripe(k, m, sb, rate="default"):
    """(clean originals, oracle recovery) of one stripe, computed once, read-only."""
    rng = np.random.default_rng(1000 * k + m + sb)
    original = rng.integers(0, 256, (k, sb), dtype=np.uint8)
    recovery = O.encode(k, m, original, rate)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


class Guarded:
    """A device output array of n bytes at offset `off` of a buffer, 0xFF before
    and behind it, pre-filled 0xA5."""

    def __init__(self, eng, n, off, pad=8):
        self.n, self.off = n, off
        self.host = np.full(off + n + pad, 0xFF, np.uint8)
        self.host[off:off + n] = 0xA5
        self.d = DeviceArray.from_numpy(eng, self.host)
        self.ptr = self.d.ptr + off

    def read(self):
        got = self.d.download()
        assert (got[:self.off] == 0xFF).all() and (got[self.off + self.n:] == 0xFF).all(), "neighbour bytes written"
        return got[self.off:self.off + self.n].copy()


def upload_guarded(eng, a):
    host = np.full(a.size + GUARD, 0x5A, np.uint8)
    host[:a.size] = a.reshape(-1)
    return host, DeviceArray.from_numpy(eng, host)


def run_locate(eng, plan, sb, o, r, fix=True):
    """One rs16_locate_device call on guarded buffers: (status, shard, fix or None)."""
    B = sb // 64
    host_o, d_o = upload_guarded(eng, o)
    host_r, d_r = upload_guarded(eng, r)
    st = Guarded(eng, B, off=1)
    sh = Guarded(eng, 4 * B, off=4)
    fx = Guarded(eng, 64 * B, off=3) if fix else None
    plan.locate(sb, d_o.ptr, d_r.ptr, st.ptr, sh.ptr, fx.ptr if fix else None)
    eng.synchronize()
    assert np.array_equal(d_o.download(), host_o), "originals (or their guard) written"
    assert np.array_equal(d_r.download(), host_r), "recovery (or its guard) written"
    return st.read(), sh.read().view(np.uint32), fx.read().reshape(B, 64) if fix else None


def patterns(k, m, sb, original, recovery):
    """name -> (stored originals, stored recovery)."""
    B = sb // 64
    last = 64 * (B - 1)
    rng = np.random.default_rng(k + m)
    out = {"clean": (original, recovery)}

    def add(name, flips_o=(), flips_r=()):
        o, r = original.copy(), recovery.copy()
        for row, byte, val in flips_o:
            o[row, byte] ^= np.uint8(val)
        for row, byte, val in flips_r:
            r[row, byte] ^= np.uint8(val)
        out[name] = (o, r)

    # one bit in one original: first / last shard, first / last block, low / high half
    add("o_first_shard_first_block_low", [(0, 3, 0x01)])
    add("o_last_shard_last_block_high", [(k - 1, last + 63, 0x80)])
    add("o_first_shard_last_block_low", [(0, last + 5, 0x10)])
    add("o_last_shard_first_block_high", [(k - 1, 40, 0x04)])
    # one original wholly random: every element of every block differs
    o = original.copy()
    noise = rng.integers(0, 256, sb, dtype=np.uint8).reshape(B, 2, 32)
    noise[:, 0, :] |= 1
    o[k // 2] ^= noise.reshape(-1)
    out["o_random_shard"] = (o, recovery)
    # one recovery shard
    add("r_first", flips_r=[(0, 1, 0x02)])
    add("r_last", flips_r=[(m - 1, last + 32, 0x40), (m - 1, last + 31, 0xFF)])
    if B > 1:
        # each block on its own
        add("o_block0_r_last_block", [(k // 3, 9, 0x20)], [(m - 1, last + 7, 0x08)])
        add("o_block0_other_o_last_block", [(0, 33, 0x01), (k - 1, last + 2, 0x55)] if k > 1 else
            [(0, 33, 0x01)], [] if k > 1 else [(0, last, 1)])
    if k > 1:
        # two originals at different elements of one block
        add("two_o_one_block", [(0, 4, 0x01), (k - 1, 5, 0x01)])
        if m >= 3:
            add("two_o_one_element", [(0, last + 6, 0x01), (k - 1, last + 6, 0x02)])
    if m >= 3:
        add("o_and_r_one_element", [(k // 2, 38, 0x01)], [(1, 6, 0x07)])
    return out


#   5:3 x 2112: 264 column lanes, more than one workgroup side by side in the
#   scan and a last one with idle lanes; 3:5 x 65600: above 64 KiB the scan keeps
#   one copy of its counts instead of 16
SHAPES = [(5, 3, 64), (5, 3, 192), (3, 5, 64), (3, 5, 192), (100, 7, 192), (40, 70, 64), (300, 2, 192),
          (1000, 1000, 1088), (3000, 1000, 64), (300, 2000, 64), (5, 3, 2112), (3, 5, 65600)]
# what the constructions are built to give, beside the reference's answer
BUILT_UNLOCATABLE = {"two_o_one_block": 0, "two_o_one_element": -1, "o_and_r_one_element": 0}


@pytest.mark.parametrize("k,m,sb", SHAPES)
def test_shapes(eng, k, m, sb):
    original, recovery = stripe(k, m, sb)
    plan = plan_for(eng, k, m)
    B = sb // 64
    pats = patterns(k, m, sb, original, recovery)
    seen = set()
    # the clean stripe again at the end: nothing of a corrupted call may linger in the engine
    for name in list(pats) + ["clean"]:
        o, r = pats[name]
        want_st, want_sh, want_fx = ref_locate(k, m, o, r)
        st, sh, fx = run_locate(eng, plan, sb, o, r)
        assert np.array_equal(st, want_st), (name, st, want_st)
        assert np.array_equal(sh, want_sh), (name, sh, want_sh)
        assert np.array_equal(fx, want_fx), (name, np.flatnonzero((fx != want_fx).any(axis=1)))
        seen.update(st.tolist())
        if name == "clean":
            assert not st.any()
        if name in BUILT_UNLOCATABLE:
            assert want_st[BUILT_UNLOCATABLE[name]] == UNLOCATABLE, name
        if name == "o_random_shard":
            assert (want_st == ORIGINAL).all() and (want_sh == k // 2).all()
        if name == "o_block0_r_last_block":
            assert want_st[0] == ORIGINAL and want_st[-1] == RECOVERY and want_sh[-1] == m - 1
    assert seen == {CLEAN, ORIGINAL, RECOVERY, UNLOCATABLE}


@pytest.mark.parametrize("k,m,sb,rate", [(40, 70, 192, "high"), (40, 70, 192, "low"), (5, 3, 64, "low"),
                                         (3, 5, 64, "high")])
def test_explicit_rate(eng, k, m, sb, rate):
    """The plan's rate is the stripe's: the two rates are different codes."""
    if not rs16.supports(k, m, rate):
        pytest.fail(f"{k}:{m} must exist at the {rate} rate")
    original, recovery = stripe(k, m, sb, rate)
    plan = plan_for(eng, k, m, rate)
    pats = patterns(k, m, sb, original, recovery)
    for name in ("clean", "o_last_shard_last_block_high", "o_random_shard", "r_last", "two_o_one_block"):
        o, r = pats[name]
        want = ref_locate(k, m, o, r, rate)
        got = run_locate(eng, plan, sb, o, r)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), (name, g, w)


def test_null_fix(eng):
    k, m, sb = 100, 7, 192
    original, recovery = stripe(k, m, sb)
    o, r = patterns(k, m, sb, original, recovery)["o_block0_r_last_block"]
    want_st, want_sh, _ = ref_locate(k, m, o, r)
    st, sh, fx = run_locate(eng, plan_for(eng, k, m), sb, o, r, fix=False)
    assert fx is None
    assert np.array_equal(st, want_st) and np.array_equal(sh, want_sh)


@pytest.mark.parametrize("k,m,sb", [(5, 3, 192), (300, 2, 192), (1000, 1000, 1088), (300, 2000, 64)])
def test_fix_round_trip(eng, k, m, sb):
    """XOR the fix into the named shard on the device: the scrub then finds nothing."""
    original, recovery = stripe(k, m, sb)
    plan = plan_for(eng, k, m)
    B = sb // 64
    pats = patterns(k, m, sb, original, recovery)
    for name in ("o_random_shard", "o_block0_r_last_block" if B > 1 else "r_last", "o_last_shard_first_block_high"):
        o, r = pats[name]
        d_o, d_r = DeviceArray.from_numpy(eng, o), DeviceArray.from_numpy(eng, r)
        d_st, d_sh, d_fx = DeviceArray(eng, B), DeviceArray(eng, 4 * B), DeviceArray(eng, 64 * B)
        d_rows, d_cols = DeviceArray(eng, m), DeviceArray(eng, B)
        rs16.verify_device(k, m, sb, d_o, d_r, d_rows, d_cols, engine=eng)
        assert d_rows.download().any() and d_cols.download().any(), name
        plan.locate(sb, d_o, d_r, d_st, d_sh, d_fx)
        st, sh = d_st.download(), d_sh.download(np.uint32)
        assert set(st.tolist()) <= {CLEAN, ORIGINAL, RECOVERY} and st.any(), name
        for c in np.flatnonzero(st):
            base = d_o.ptr if st[c] == ORIGINAL else d_r.ptr
            eng.xor(base + int(sh[c]) * sb + 64 * int(c), d_fx.ptr + 64 * int(c), 64)
        rs16.verify_device(k, m, sb, d_o, d_r, d_rows, d_cols, engine=eng)
        assert not d_rows.download().any() and not d_cols.download().any(), name
        assert np.array_equal(d_o.download(shape=(k, sb)), original), name
        assert np.array_equal(d_r.download(shape=(m, sb)), recovery), name


def test_largest_shape(eng):
    """32768:32768 x 64 B: 64 plan chunks, shard indices that need all 15 bits.
    Expected values from the construction: one flipped bit of one shard."""
    k = m = 32768
    sb = 64
    original, recovery = stripe(k, m, sb)
    plan = plan_for(eng, k, m)
    st, sh, fx = run_locate(eng, plan, sb, original, recovery)
    assert st.tolist() == [CLEAN] and sh.tolist() == [NO_SHARD] and not fx.any()
    for row, byte, val in ((0, 0, 0x01), (511, 31, 0x80), (512, 32, 0x01), (16385, 17, 0x10), (k - 1, 63, 0x40)):
        o = original.copy()
        o[row, byte] ^= np.uint8(val)
        st, sh, fx = run_locate(eng, plan, sb, o, recovery)
        assert st.tolist() == [ORIGINAL] and sh.tolist() == [row], (row, st, sh)
        assert np.array_equal(fx[0], o[row] ^ original[row]), row
    for row, byte, val in ((0, 5, 0x02), (m - 1, 63, 0x80)):
        r = recovery.copy()
        r[row, byte] ^= np.uint8(val)
        st, sh, fx = run_locate(eng, plan, sb, original, r)
        assert st.tolist() == [RECOVERY] and sh.tolist() == [row], (row, st, sh)
        assert np.array_equal(fx[0], r[row] ^ recovery[row]), row
    # two originals at different elements of the block
    o = original.copy()
    o[1, 2] ^= 1
    o[k - 2, 3] ^= 1
    st, sh, fx = run_locate(eng, plan, sb, o, recovery)
    assert st.tolist() == [UNLOCATABLE] and sh.tolist() == [NO_SHARD] and not fx.any()
    st, sh, fx = run_locate(eng, plan, sb, original, recovery)
    assert st.tolist() == [CLEAN] and sh.tolist() == [NO_SHARD] and not fx.any()


@pytest.mark.parametrize("k,m,rate", [(5, 3, "high"), (5, 3, "low"), (3, 5, "low"), (3, 5, "high"), (100, 7, "default"),
                                      (40, 70, "default"), (1000, 1000, "default"), (3000, 1000, "high"),
                                      (300, 2000, "low"), (300, 2, "default")])
def test_plan_rows_are_the_oracle_matrix(eng, k, m, rate):
    rows = plan_for(eng, k, m, rate).rows()
    assert np.array_equal(rows, matrix(k, m, rate)[:2])


def test_host_level_locate(eng):
    k, m, sb = 100, 7, 192
    original, recovery = stripe(k, m, sb)
    o, r = patterns(k, m, sb, original, recovery)["o_block0_r_last_block"]
    st, sh, fx = rs16.locate(k, m, list(o), list(r), engine=eng)
    want = ref_locate(k, m, o, r)
    assert st.dtype == np.uint8 and sh.dtype == np.uint32 and fx.shape == (sb // 64, 64)
    for g, w in zip((st, sh, fx), want):
        assert np.array_equal(g, w)
    st, sh, fx = rs16.locate(k, m, original, recovery, engine=eng)
    assert not st.any() and (sh == rs16.LOCATE_NO_SHARD).all() and not fx.any()
    assert (rs16.LOCATE_CLEAN, rs16.LOCATE_ORIGINAL, rs16.LOCATE_RECOVERY, rs16.LOCATE_UNLOCATABLE) == \
        (CLEAN, ORIGINAL, RECOVERY, UNLOCATABLE)


def plan_new(eng, rate, k, m):
    err = RS16Error()
    h = lib().rs16_locate_plan_new(eng.h, rate, k, m, C.byref(err))
    if h:
        lib().rs16_locate_plan_free(h)
        return None
    return rs16.Error._from_c(err).kind


def call(plan_h, sb, o, r, st, sh, fx=None):
    err = RS16Error()
    rc = lib().rs16_locate_device(plan_h, sb, o, r, st, sh, fx, None, C.byref(err))
    return rs16.Error._from_c(err).kind if rc else None


def test_errors_in_order(eng):
    # the plan: unsupported counts first, then recovery_count < 2
    assert plan_new(eng, 0, 0, 1) == "UnsupportedShardCount"
    assert plan_new(eng, 0, 40000, 40000) == "UnsupportedShardCount"
    assert plan_new(eng, 1, 4096, 61440) == "UnsupportedShardCount"
    assert plan_new(eng, 0, 5, 1) == "InvalidArgument"
    assert plan_new(eng, 2, 1, 1) == "InvalidArgument"
    assert plan_new(eng, 0, 1, 2) is None
    k, m, sb = 100, 7, 64
    plan = plan_for(eng, k, m)
    d = DeviceArray(eng, k * sb + 128)
    f = DeviceArray(eng, 1024)
    # no plan: whatever else is wrong
    assert call(None, 100, None, None, None, None) == "InvalidArgument"
    # then the shard size
    assert call(plan.h, 0, None, d.ptr + 1, None, None) == "InvalidShardSize"
    assert call(plan.h, 100, None, d.ptr + 1, None, None) == "InvalidShardSize"
    assert call(plan.h, 2**32, d.ptr, d.ptr, f.ptr, f.ptr + 64) == "InvalidShardSize"
    # then the arguments
    assert call(plan.h, sb, None, d.ptr, f.ptr, f.ptr + 64) == "InvalidArgument"
    assert call(plan.h, sb, d.ptr, None, f.ptr, f.ptr + 64) == "InvalidArgument"
    assert call(plan.h, sb, d.ptr + 32, d.ptr, f.ptr, f.ptr + 64) == "InvalidArgument"
    assert call(plan.h, sb, d.ptr, d.ptr + 16, f.ptr, f.ptr + 64) == "InvalidArgument"
    assert call(plan.h, sb, d.ptr, d.ptr, None, f.ptr + 64) == "InvalidArgument"
    assert call(plan.h, sb, d.ptr, d.ptr, f.ptr, None) == "InvalidArgument"
    err = RS16Error()
    assert lib().rs16_locate_plan_rows(plan.h, None, C.byref(err)) != 0
    assert lib().rs16_locate_plan_rows(None, None, C.byref(err)) != 0


def test_detached_plan_fails_after_engine_free():
    e2 = rs16.Engine(0)
    plan = rs16.LocatePlan(5, 3, engine=e2)
    d = DeviceArray(e2, 5 * 64)
    f = DeviceArray(e2, 256)
    assert call(plan.h, 64, d.ptr, d.ptr, f.ptr, f.ptr + 64, f.ptr + 128) is None
    e2.synchronize()
    ptrs = (d.ptr, f.ptr)
    e2.close()
    assert call(plan.h, 64, ptrs[0], ptrs[0], ptrs[1], ptrs[1] + 64) == "InvalidArgument"
    out = np.zeros(10, np.uint16)
    err = RS16Error()
    assert lib().rs16_locate_plan_rows(plan.h, out.ctypes.data_as(C.POINTER(C.c_uint16)), C.byref(err)) != 0
    with pytest.raises(rs16.Error):
        plan.locate(64, ptrs[0], ptrs[0], ptrs[1], ptrs[1] + 64)
    plan.close()  # frees host memory only
    plan.close()


def test_locate_keeps_decode_state(eng):
    """Like the scrub, a locate is not a decode: a pending rs16_decode_prepare
    survives it and rs16_decode_check still reports the last decode."""
    k, m, sb = 100, 100, 192
    original, recovery = stripe(k, m, sb)
    plan = plan_for(eng, k, m)
    o, r = patterns(k, m, sb, original, recovery)["o_block0_r_last_block"]
    want = ref_locate(k, m, o, r)

    def locate_ok():
        got = run_locate(eng, plan, sb, o, r)
        for g, w in zip(got, want):
            assert np.array_equal(g, w)

    of = np.ones(k, np.uint8)
    of[[1, 50, 99]] = 0
    held = original.copy()
    held[of == 0] = 0xA5
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, recovery)
    d_fo, d_fr = DeviceArray.from_numpy(eng, of), DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    # a locate between the prepare and the prepared decode
    rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, k - 3, m, engine=eng)
    locate_ok()
    rs16.decode_device_prepared(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_o.download(shape=(k, sb)), original)
    # a decode given a wrong count, then a locate: rs16_decode_check still reports that decode
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 2, m, engine=eng)
    locate_ok()
    err = RS16Error()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) != 0
    assert (err.v0, err.v1) == (k - 3, m)
    d_o.upload(held)
    rs16.decode_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 3, m, engine=eng)
    locate_ok()
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) == 0
