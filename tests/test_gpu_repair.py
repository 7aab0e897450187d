"""rs16_repair_device / rs16_repair_device_batch (include/rs16.h): a decode with
d_recovery writable -- lost originals restored and lost recovery shards
regenerated, both in place.

Expected values: the originals are the test's own data, the recovery shards
are the oracle's encode of them (the algebra that makes the decode's work rows
carry them: tests/test_repair_path.py).  Every case pre-fills the lost slots
of both arrays with 0xA5 and checks both arrays whole -- lost slots exact,
received slots byte-identical -- and a 64-byte guard block behind each.

One shape per kernel geometry (the one-pass kernel at its tile sizes and both
rates, the three-pass form at every tile size 2^4 .. 2^8, a tile that holds
rows of both segments, multi-chunk encoders behind the recovery-only path),
and per shape the loss patterns (a) .. (f) below where at least
original_count shards remain.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, sb, seed=0):
    """(originals, oracle recovery) of one stripe, computed once, read-only."""
    original = generate_original(k, sb, 7 * k + m + seed)
    recovery = O.encode(k, m, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def pattern(k, m, name):
    """(originals received, recovery received) as bool arrays."""
    ok = np.ones(k + m, bool)
    rng = np.random.default_rng(100 * k + m)
    if name == "a":      # original 0 and the last recovery shard
        ok[[0, k + m - 1]] = False
    elif name == "b":    # the last original and recovery 0
        ok[[k - 1, k]] = False
    elif name == "c":    # exactly original_count received, losses over both kinds at random
        lost = rng.choice(k + m, m, replace=False)
        if m >= 2 and (lost < k).all():
            lost[0] = k + int(rng.integers(m))
        if m >= 2 and (lost >= k).all():
            lost[0] = int(rng.integers(k))
        ok[lost] = False
        ok[rng.choice(np.flatnonzero(ok), int(ok.sum()) - k, replace=False)] = False  # (a replaced duplicate)
    elif name == "d":    # a run across the original / recovery boundary: the failed device
        r = max(1, min(k, m) // 4)
        ok[k - r:k + r] = False
    elif name == "e":    # recovery shards only: encode + copy
        ok[[k, k + m // 2, k + m - 1]] = False
    elif name == "f":    # originals only: the decode
        ok[sorted({0, k // 2, k - 1})[:m]] = False
    return ok[:k], ok[k:]


def upload(eng, k, m, sb, ok_o, ok_r, recv=(1, 1), seed=0):
    original, recovery = stripe(k, m, sb, seed)
    host_o = np.full(k * sb + GUARD, 0x5A, np.uint8)
    host_r = np.full(m * sb + GUARD, 0x5A, np.uint8)
    ho, hr = host_o[:k * sb].reshape(k, sb), host_r[:m * sb].reshape(m, sb)
    ho[:], hr[:] = original, recovery
    ho[~ok_o] = 0xA5
    hr[~ok_r] = 0xA5
    # any nonzero flag byte means received
    fo = np.where(ok_o, np.where(np.arange(k) % 2 == 0, recv[0], recv[1]), 0).astype(np.uint8)
    fr = np.where(ok_r, np.where(np.arange(m) % 2 == 0, recv[1], recv[0]), 0).astype(np.uint8)
    return (DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, host_r),
            DeviceArray.from_numpy(eng, fo), DeviceArray.from_numpy(eng, fr))


def check_whole(d_o, d_r, k, m, sb, seed=0):
    original, recovery = stripe(k, m, sb, seed)
    got_o, got_r = d_o.download(), d_r.download()
    assert (got_o[k * sb:] == 0x5A).all() and (got_r[m * sb:] == 0x5A).all(), "guard block written"
    bad_o = np.flatnonzero((got_o[:k * sb].reshape(k, sb) != original).any(axis=1))
    bad_r = np.flatnonzero((got_r[:m * sb].reshape(m, sb) != recovery).any(axis=1))
    assert bad_o.size == 0 and bad_r.size == 0, (bad_o[:8], bad_r[:8])


def repair(eng, k, m, sb, ok_o, ok_r, **kw):
    d_o, d_r, d_fo, d_fr = upload(eng, k, m, sb, ok_o, ok_r, **kw)
    rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, int(ok_o.sum()), int(ok_r.sum()), engine=eng,
                       check=True)
    return d_o, d_r


SHAPES = [(1, 1), (3, 2), (2, 3), (100, 100), (40, 200), (200, 200), (600, 300), (3000, 5), (5, 3000), (1000, 100),
          (8000, 8000), (30000, 30000), (32768, 32768)]
LOW_RATE = {(2, 3), (40, 200), (5, 3000)}
ROWS = {(100, 100): 256, (200, 200): 512, (600, 300): 2048, (8000, 8000): 16384, (30000, 30000): 65536,
        (32768, 32768): 65536}


def _cases():
    for k, m in SHAPES:
        for name in "abcdef":
            ok_o, ok_r = pattern(k, m, name)
            if ok_o.sum() + ok_r.sum() < k:
                continue  # (1:1 cannot lose a shard of each kind)
            yield pytest.param(k, m, name, id=f"{k}:{m}-{name}")


def test_shapes_are_what_they_stand_for():
    for k, m in SHAPES:
        high = bool(rs16.use_high_rate(k, m))
        assert high == ((k, m) not in LOW_RATE), (k, m)
        if (k, m) in ROWS:
            assert lib().rs16_decoder_work_count(1 if high else 0, k, m) == ROWS[(k, m)]
    # the last pass's tile sizes 2^4 .. 2^8, and a tile with rows of both segments
    los = {(k, m): rs16.repair_path(k, m, k - 1, m - 1)[1] for k, m in SHAPES if (k, m) != (1, 1)}
    assert (los[(40, 200)], los[(200, 200)], los[(600, 300)], los[(3000, 5)], los[(5, 3000)], los[(1000, 100)],
            los[(8000, 8000)], los[(30000, 30000)], los[(32768, 32768)]) == (4, 4, 5, 6, 6, 5, 7, 8, 8)
    assert all(los[s] == 0 for s in [(3, 2), (2, 3), (100, 100)])  # the one-pass kernel


@pytest.mark.parametrize("k,m,name", list(_cases()))
def test_repair(eng, k, m, name):
    sb = 64
    ok_o, ok_r = pattern(k, m, name)
    want_path = 3 if (not ok_o.all() and not ok_r.all()) else (2 if ok_o.all() else 1)
    assert rs16.repair_path(k, m, int(ok_o.sum()), int(ok_r.sum()))[0] == want_path
    if name in "abcd" and (k, m) != (1, 1):
        assert want_path == 3
    d_o, d_r = repair(eng, k, m, sb, ok_o, ok_r)
    check_whole(d_o, d_r, k, m, sb)
    if name == "f":
        # no recovery shard lost: the decode itself, the same bytes
        x_o, x_r, x_fo, x_fr = upload(eng, k, m, sb, ok_o, ok_r)
        rs16.decode_device(k, m, sb, x_o.ptr, x_fo.ptr, x_r.ptr, x_fr.ptr, int(ok_o.sum()), int(ok_r.sum()),
                           engine=eng)
        assert np.array_equal(x_o.download(), d_o.download()) and np.array_equal(x_r.download(), d_r.download())


@pytest.mark.parametrize("k,m,sb,name", [
    (600, 300, 2048, "c"), (600, 300, 2048, "d"), (600, 300, 2048, "e"),
    (30000, 30000, 192, "d"), (30000, 30000, 192, "a"), (30000, 30000, 192, "e"),  # no power of two
])
def test_widths(eng, k, m, sb, name):
    ok_o, ok_r = pattern(k, m, name)
    d_o, d_r = repair(eng, k, m, sb, ok_o, ok_r)
    check_whole(d_o, d_r, k, m, sb)


@pytest.mark.parametrize("k,m,name", [(200, 200, "c"), (200, 200, "e"), (3000, 5, "a"), (100, 100, "d")])
def test_flag_bytes(eng, k, m, name):
    ok_o, ok_r = pattern(k, m, name)
    d_o, d_r = repair(eng, k, m, 64, ok_o, ok_r, recv=(0x80, 0xFF))
    check_whole(d_o, d_r, k, m, 64)


@pytest.mark.parametrize("k,m,recv,nstripes", [(200, 200, (1, 1), 1), (200, 200, (0x80, 0xFF), 1),
                                               (1000, 100, (2, 0x40), 1), (5, 3000, (0xFF, 0x80), 1),
                                               (200, 200, (0x80, 0xFF), 3), (5, 3000, (0xFF, 0x80), 2)])
def test_recovery_only_writes_no_received_slot(eng, k, m, recv, nstripes):
    """Path 2 reads no recovery shard, so the received recovery slots can hold
    anything: here junk that the encode would not produce.  A copy that ignored
    the flags, or took only the value 1 for "received", would overwrite it."""
    sb, gap = 64, 128
    ok_o, ok_r = pattern(k, m, "e")
    assert rs16.repair_path(k, m, k, int(ok_r.sum()))[0] == 2
    sr, so = m * sb + gap, k * sb
    host_o = np.concatenate([stripe(k, m, sb, seed=i)[0].reshape(-1) for i in range(nstripes)])
    junk = np.random.default_rng(k + m).integers(0, 256, nstripes * sr + GUARD, dtype=np.uint8)
    d_o, d_r = DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, junk)
    fo = np.where(np.arange(k) % 2 == 0, recv[0], recv[1]).astype(np.uint8)
    fr = np.where(ok_r, np.where(np.arange(m) % 2 == 0, recv[1], recv[0]), 0).astype(np.uint8)
    d_fo, d_fr = DeviceArray.from_numpy(eng, fo), DeviceArray.from_numpy(eng, fr)
    if nstripes == 1:
        rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k, int(ok_r.sum()), engine=eng)
    else:
        rs16.repair_device_batch(k, m, sb, nstripes, d_o.ptr, so, d_fo.ptr, d_r.ptr, sr, d_fr.ptr, k,
                                 int(ok_r.sum()), engine=eng)
    got = d_r.download()
    want = junk.copy()
    for i in range(nstripes):
        w = want[i * sr:i * sr + m * sb].reshape(m, sb)
        w[~ok_r] = stripe(k, m, sb, seed=i)[1][~ok_r]  # the lost rows regenerated, nothing else
    assert np.array_equal(got, want)
    assert np.array_equal(d_o.download(), host_o)


@pytest.mark.parametrize("k,m,name", [(200, 200, "d"), (200, 200, "e"), (200, 200, "f"), (3000, 5, "d"),
                                      (3000, 5, "e"), (3000, 5, "b"), (5, 3000, "d"), (5, 3000, "e")])
def test_batch(eng, k, m, name):
    sb, n, gap = 64, 3, 128
    so, sr = k * sb + gap, m * sb + gap
    ok_o, ok_r = pattern(k, m, name)
    host_o = np.full(n * so + GUARD, 0x5A, np.uint8)
    host_r = np.full(n * sr + GUARD, 0x5A, np.uint8)
    singles = []
    for i in range(n):
        original, recovery = stripe(k, m, sb, seed=i)
        ho = host_o[i * so:i * so + k * sb].reshape(k, sb)
        hr = host_r[i * sr:i * sr + m * sb].reshape(m, sb)
        ho[:], hr[:] = original, recovery
        ho[~ok_o] = 0xA5
        hr[~ok_r] = 0xA5
        s_o, s_r = repair(eng, k, m, sb, ok_o, ok_r, seed=i)  # the single call on this stripe
        singles.append((s_o.download()[:k * sb], s_r.download()[:m * sb]))
    d_o, d_r = DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, host_r)
    d_fo = DeviceArray.from_numpy(eng, ok_o.astype(np.uint8))
    d_fr = DeviceArray.from_numpy(eng, ok_r.astype(np.uint8))
    rs16.repair_device_batch(k, m, sb, n, d_o.ptr, so, d_fo.ptr, d_r.ptr, sr, d_fr.ptr, int(ok_o.sum()),
                             int(ok_r.sum()), engine=eng)
    got_o, got_r = d_o.download(), d_r.download()
    for i in range(n):
        original, recovery = stripe(k, m, sb, seed=i)
        assert np.array_equal(got_o[i * so:i * so + k * sb], singles[i][0]), i
        assert np.array_equal(got_r[i * sr:i * sr + m * sb], singles[i][1]), i
        assert np.array_equal(got_o[i * so:i * so + k * sb].reshape(k, sb), original), i
        assert np.array_equal(got_r[i * sr:i * sr + m * sb].reshape(m, sb), recovery), i
        assert (got_o[i * so + k * sb:(i + 1) * so] == 0x5A).all(), i  # gap bytes untouched
        assert (got_r[i * sr + m * sb:(i + 1) * sr] == 0x5A).all(), i
    assert (got_o[n * so:] == 0x5A).all() and (got_r[n * sr:] == 0x5A).all()


def test_errors_and_their_order(eng):
    k, m, sb = 4, 4, 64
    d_o, d_r = DeviceArray(eng, 2 * k * sb + 64), DeviceArray(eng, 2 * m * sb + 64)
    f = DeviceArray.from_numpy(eng, np.ones(8, np.uint8))

    def single(**kw):
        a = dict(k=k, m=m, sb=sb, o=d_o.ptr, fo=f.ptr, r=d_r.ptr, fr=f.ptr, no=k - 1, nr=m - 1)
        a.update(kw)
        return lambda: rs16.repair_device(a["k"], a["m"], a["sb"], a["o"], a["fo"], a["r"], a["fr"], a["no"],
                                          a["nr"], engine=eng)

    def batch(**kw):
        a = dict(k=k, m=m, sb=sb, n=2, o=d_o.ptr, so=k * sb, fo=f.ptr, r=d_r.ptr, sr=m * sb, fr=f.ptr, no=k - 1,
                 nr=m - 1)
        a.update(kw)
        return lambda: rs16.repair_device_batch(a["k"], a["m"], a["sb"], a["n"], a["o"], a["so"], a["fo"], a["r"],
                                                a["sr"], a["fr"], a["no"], a["nr"], engine=eng)

    def kind(call):
        with pytest.raises(rs16.Error) as e:
            call()
        return e.value

    for form in (single, batch):
        # rs16_validate's errors first, whatever else is wrong
        assert kind(form(k=0, o=0)) == rs16.Error("UnsupportedShardCount", original_count=0, recovery_count=m)
        assert kind(form(k=40000, m=40000, no=0, nr=0)).kind == "UnsupportedShardCount"
        assert kind(form(sb=100, o=d_o.ptr + 32, no=0, nr=0)) == rs16.Error("InvalidShardSize", shard_bytes=100)
        assert kind(form(sb=0)).kind == "InvalidShardSize"
        # null / misaligned arrays, before the counts are looked at
        for bad in (dict(o=0), dict(r=0), dict(fo=0), dict(fr=0), dict(o=d_o.ptr + 32), dict(r=d_r.ptr + 16)):
            assert kind(form(no=0, nr=0, **bad)).kind == "InvalidArgument", bad
        # counts: above the shard count, then too few
        assert kind(form(no=k + 1)).kind == "InvalidArgument"
        assert kind(form(nr=m + 1)).kind == "InvalidArgument"
        assert kind(form(no=1, nr=2)) == rs16.Error("NotEnoughShards", original_count=k, original_received_count=1,
                                                    recovery_received_count=2)
    # bad strides, before the counts
    for bad in (dict(so=k * sb - 64), dict(sr=m * sb - 64), dict(so=k * sb + 32), dict(sr=m * sb + 32)):
        assert kind(batch(no=0, nr=0, **bad)).kind == "InvalidArgument", bad
    # no stripes: nothing to do once the arguments are valid
    batch(n=0)()


def test_everything_received_changes_nothing(eng):
    k, m, sb = 200, 200, 64
    ok_o, ok_r = np.ones(k, bool), np.ones(m, bool)
    d_o, d_r, d_fo, d_fr = upload(eng, k, m, sb, ok_o, ok_r)
    # (not the stripe's own recovery: a repair that re-encoded would show)
    junk = np.full(m * sb + GUARD, 0x33, np.uint8)
    d_r.upload(junk)
    before = d_o.download()
    eng.set_profiling(True)
    try:
        rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k, m, engine=eng)
        rs16.repair_device_batch(k, m, sb, 1, d_o.ptr, k * sb, d_fo.ptr, d_r.ptr, m * sb, d_fr.ptr, k, m, engine=eng)
        launches = {n: c for n, (_, c) in eng.profile().items() if c}
    finally:
        eng.set_profiling(False)
    assert launches == {}, launches  # nothing launched
    assert np.array_equal(d_o.download(), before) and np.array_equal(d_r.download(), junk)


def test_programs_launched(eng):
    """Path 3 runs the new last pass / one-pass program, path 2 the encode and the copy."""
    def progs(k, m, name):
        ok_o, ok_r = pattern(k, m, name)
        d_o, d_r, d_fo, d_fr = upload(eng, k, m, 64, ok_o, ok_r)
        eng.profile_reset()
        eng.set_profiling(True)
        try:
            rs16.repair_device(k, m, 64, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, int(ok_o.sum()), int(ok_r.sum()),
                               engine=eng)
            got = {n: c for n, (_, c) in eng.profile().items() if c}
        finally:
            eng.set_profiling(False)
        check_whole(d_o, d_r, k, m, 64)
        return got

    assert progs(100, 100, "a") == {"EVAL_POLY": 1, "DEC_SINGLE_ALL": 1}
    # 200:200 is a column-codec stripe for the decode; the repair takes the passes, two last-pass launches
    assert progs(200, 200, "a") == {"EVAL_POLY": 1, "DEC_FIRST": 1, "DEC_MID": 1, "DEC_LAST_ALL": 2}
    assert progs(3000, 5, "a") == {"EVAL_POLY": 1, "DEC_FIRST": 1, "DEC_MID": 1, "DEC_LAST_ALL": 1}
    assert progs(32768, 32768, "d") == {"EVAL_POLY": 1, "DEC_FIRST": 1, "DEC_MID": 1, "DEC_LAST_ALL": 1}
    got = progs(8000, 8000, "e")
    assert got.pop("REPAIR_COPY") == 1 and not any(n.startswith("DEC_") or n == "EVAL_POLY" for n in got), got


def test_decode_check(eng):
    k, m, sb = 200, 200, 64
    ok_o, ok_r = pattern(k, m, "a")
    d_o, d_r, d_fo, d_fr = upload(eng, k, m, sb, ok_o, ok_r)
    err = RS16Error()
    rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - 1, m - 1, engine=eng)
    assert lib().rs16_decode_check(eng.h, None, C.byref(err)) == 0
    check_whole(d_o, d_r, k, m, sb)
    # a recovery count one too high is still a valid decode; the flags say otherwise
    d_o, d_r, d_fo, d_fr = upload(eng, k, m, sb, *pattern(k, m, "d"))
    lost = k - int(pattern(k, m, "d")[0].sum())
    rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, k - lost, m - lost + 1, engine=eng)
    rc = lib().rs16_decode_check(eng.h, None, C.byref(err))
    assert rs16.Error._from_c(err).kind == "InvalidArgument" and rc == err.code
    assert (err.v0, err.v1) == (k - lost, m - lost)


def test_repair_discards_a_preparation(eng):
    k, m, sb = 2000, 2000, 64
    ok_o, ok_r = pattern(k, m, "d")
    d_o, d_r, d_fo, d_fr = upload(eng, k, m, sb, ok_o, ok_r)
    no, nr = int(ok_o.sum()), int(ok_r.sum())
    rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, no, nr, engine=eng)
    rs16.repair_device(k, m, sb, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, no, nr, engine=eng)
    check_whole(d_o, d_r, k, m, sb)
    with pytest.raises(rs16.Error) as e:
        rs16.decode_device_prepared(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert e.value.kind == "InvalidArgument"


def test_lifecycle_repair_leaves_no_path_state():
    """repair -> encode -> decodes of every kind on one engine, each correct."""
    eng = rs16.Engine(0)
    try:
        k = m = 4096
        sb = 64
        original, recovery = stripe(k, m, sb)
        d_o, d_r = repair(eng, k, m, sb, *pattern(k, m, "c"))
        check_whole(d_o, d_r, k, m, sb)
        # encode
        x_r = DeviceArray(eng, m * sb)
        rs16.encode_device(k, m, sb, d_o.ptr, x_r.ptr, engine=eng)
        assert np.array_equal(x_r.download(shape=(m, sb)), recovery)
        # every original lost: the identity decode (DecodePlan::ident)
        d_fo = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
        d_fr = DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
        d_x = DeviceArray.from_numpy(eng, np.full((k, sb), 0xA5, np.uint8))
        rs16.decode_device(k, m, sb, d_x.ptr, d_fo.ptr, x_r.ptr, d_fr.ptr, 0, m, engine=eng, check=True)
        assert np.array_equal(d_x.download(shape=(k, sb)), original)
        # the repair again, then a general decode and a column-codec decode (DecodePlan::eval_in_col)
        d_o, d_r = repair(eng, k, m, sb, *pattern(k, m, "d"))
        check_whole(d_o, d_r, k, m, sb)
        for kk, mm in ((4096, 4096), (1000, 1000)):
            ok_o, _ = pattern(kk, mm, "f")
            ok_r = np.zeros(mm, bool)
            ok_r[:int((~ok_o).sum())] = True
            y_o, y_r, y_fo, y_fr = upload(eng, kk, mm, sb, ok_o, np.ones(mm, bool))
            y_fr.upload(ok_r.astype(np.uint8))
            rs16.decode_device(kk, mm, sb, y_o.ptr, y_fo.ptr, y_r.ptr, y_fr.ptr, int(ok_o.sum()), int(ok_r.sum()),
                               engine=eng, check=True)
            check_whole(y_o, y_r, kk, mm, sb)
        # ... and a repair in the size the column decode just ran at
        d_o, d_r = repair(eng, 1000, 1000, sb, *pattern(1000, 1000, "a"))
        check_whole(d_o, d_r, 1000, 1000, sb)
    finally:
        eng.close()
