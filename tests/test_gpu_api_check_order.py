"""The ORDER of the argument checks of the one-shot decode / batch entry points
(include/rs16.h): a call with two faults reports the one its entry point looks
for first, and that order is part of what a caller sees.  The single-fault
cases live with each entry point's own tests (test_gpu_batch.py,
test_gpu_host_path.py, test_gpu_prepared.py, test_gpu_flag_bytes.py); here
every case carries two faults, or a fault next to a "nothing to do" condition,
at the smallest geometry (k = 4, m = 2: high rate; S = 64; at most two
stripes), through the raw C ABI.

The order, per entry point:
  rs16_decode_device               rate/shape, counts above k or m, NotEnoughShards, misaligned array,
                                   nothing to restore (OK)
  rs16_decode_device_batch         rate, count range, NotEnoughShards, nstripes == 0 (OK), misaligned,
                                   nothing to restore (OK), NULL / stride / nstripes > 2^20
  rs16_decode_device_batch_varied  rate, nstripes == 0 (OK), every pointer / stride / alignment fault,
                                   then per stripe range before NotEnoughShards, the first such stripe
  rs16_encode_device_batch         rate, nstripes == 0 (OK), stride / alignment
  rs16_decode_prepare              a failed call of any kind leaves no valid preparation
  rs16_decode_host, _host_batch, _host_multi
                                   (multi: NULL engine,) rate, (batch: nstripes == 0, NULL / stride,)
                                   NotEnoughShards of the first such stripe, nothing lost (OK, no device work)
No case launches a kernel except the valid preparation of test_prepare."""
import ctypes as C

import numpy as np
import pytest

import rs16
from rs16._lib import RS16Error, lib
from rs16.device import DeviceArray

pytestmark = pytest.mark.gpu

K, M, S = 4, 2, 64
OK, SHARD_SIZE, NOT_ENOUGH, INVALID = 0, 6, 7, 101
BAD_S = 100  # no multiple of 64: RS16_INVALID_SHARD_SIZE from the rate check
BIG = (1 << 20) + 1


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dev(eng):
    """(originals, recovery, original flags, recovery flags): device addresses
    of two stripes' worth of shard rows (64-byte aligned) and of the flags
    1,1,1,0 / 1,0 of each stripe (flag stride 8), with a guard copy."""
    guard = (np.arange(4096) * 37 % 251).astype(np.uint8)
    d = DeviceArray.from_numpy(eng, guard)
    f = DeviceArray.from_numpy(eng, np.array([0x80, 2, 0xFF, 0, 0, 0, 0, 0, 1, 0x40, 0x7F, 0, 0, 0, 0, 0,
                                              0xFE, 0, 0, 0, 0, 0, 0, 0, 0xAA, 0, 0, 0, 0, 0, 0, 0], np.uint8))
    assert d.ptr % 64 == 0
    yield d.ptr, d.ptr + 2048, f.ptr, f.ptr + 16
    eng.synchronize()
    assert np.array_equal(d.download(), guard), "a refused or empty call wrote device memory"


def call(name, *args):
    """(code, v0, v1, v2) of one raw C-ABI call; the return value is the code."""
    err = RS16Error()
    rc = getattr(lib(), name)(*args, C.byref(err))
    assert rc == err.code, (name, rc, err.code)
    return err.code, err.v0, err.v1, err.v2


def counts(*v):
    return (C.c_size_t * len(v))(*v)


def few(o, r):
    return (NOT_ENOUGH, K, o, r)


def test_decode_device(eng, dev):
    A, B, fo, fr = dev

    def dec(s, a, b, o, r):
        return call("rs16_decode_device", eng.h, K, M, s, a, fo, b, fr, o, r, None)

    assert dec(BAD_S, A + 8, B, 5, 0)[0] == SHARD_SIZE    # rate before range and alignment
    assert dec(BAD_S, A, B, 0, 1)[0] == SHARD_SIZE        # rate before NotEnoughShards
    assert dec(S, A, B, 0, 3)[0] == INVALID               # range (3 > m) before NotEnoughShards (0 + 3 < 4)
    assert dec(S, A + 8, B, 1, 1) == few(1, 1)            # NotEnoughShards before misaligned
    assert dec(S, A, B + 32, 1, 1) == few(1, 1)
    assert dec(S, A + 16, B, 4, 0)[0] == INVALID          # misaligned before nothing to restore
    assert dec(S, A, B + 16, 4, 2)[0] == INVALID
    assert dec(S, A, B, 4, 0)[0] == OK
    eng.synchronize()


def test_decode_device_batch(eng, dev):
    A, B, fo, fr = dev

    def dec(s, n, a, so, b, sr, o, r):
        return call("rs16_decode_device_batch", eng.h, K, M, s, n, a, so, fo, b, sr, fr, o, r, None)

    so, sr = K * S, M * S
    assert dec(BAD_S, 0, A, so, B, sr, 3, 1)[0] == SHARD_SIZE    # rate before nstripes == 0
    assert dec(S, 0, A, so, B, sr, 0, 3)[0] == INVALID           # range before nstripes == 0
    assert dec(S, 0, A, so, B, sr, 1, 1) == few(1, 1)            # NotEnoughShards before nstripes == 0
    assert dec(S, 2, A + 8, 64, B, sr, 1, 1) == few(1, 1)        # ... before misaligned and stride
    assert dec(S, 0, A + 8, 64, None, 0, 3, 1)[0] == OK          # nstripes == 0 before every array fault
    assert dec(S, 2, A + 8, so, B, sr, 4, 0)[0] == INVALID       # misaligned before nothing to restore
    assert dec(S, 2, A, 64, B, 32, 4, 0)[0] == OK                # nothing to restore before the strides,
    assert dec(S, 2, None, 0, None, 0, 4, 1)[0] == OK            # ... NULL
    assert dec(S, BIG, A, so, B, sr, 4, 0)[0] == OK              # ... and nstripes > 2^20
    assert dec(S, 2, A, 64, B, sr, 3, 1)[0] == INVALID           # (the same faults with a shard to restore)
    assert dec(S, 2, A, so, B, sr + 32, 3, 1)[0] == INVALID
    assert dec(S, BIG, A, so, B, sr, 3, 1)[0] == INVALID
    eng.synchronize()


def test_decode_device_batch_varied(eng, dev):
    A, B, fo, fr = dev

    def dec(s, n, a, so, fso, b, sr, fsr, oc, rc, f_o=fo, f_r=fr):
        return call("rs16_decode_device_batch_varied", eng.h, K, M, s, n, a, so, f_o, fso, b, sr, f_r, fsr, oc, rc,
                    None)

    so, sr = K * S, M * S
    good = counts(3, 3), counts(1, 1)
    assert dec(BAD_S, 0, A, so, 8, B, sr, 8, *good)[0] == SHARD_SIZE       # rate before nstripes == 0
    assert dec(S, 0, None, 0, 0, None, 0, 0, None, None, None, None)[0] == OK  # nstripes == 0 before the rest
    lacking = counts(1, 3), counts(1, 1)
    assert dec(S, 2, A, 64, 8, B, sr, 8, *lacking)[0] == INVALID           # stride before NotEnoughShards:
    assert dec(S, 2, A + 8, so, 8, B, sr, 8, *lacking)[0] == INVALID       # ... misaligned,
    assert dec(S, 2, A, so, 3, B, sr, 8, *lacking)[0] == INVALID           # ... flag stride below k,
    assert dec(S, 2, A, so, 8, B, sr, 8, *lacking, f_r=None)[0] == INVALID  # ... NULL flags
    assert dec(S, 2, A, so, 8, B, sr, 8, *lacking) == few(1, 1)
    # per stripe, range then NotEnoughShards; the first stripe with either decides
    assert dec(S, 2, A, so, 8, B, sr, 8, counts(0, 3), counts(3, 1))[0] == INVALID   # 3 > m in a stripe short of k
    assert dec(S, 2, A, so, 8, B, sr, 8, counts(1, 5), counts(1, 0)) == few(1, 1)    # too few, then a range fault
    assert dec(S, 2, A, so, 8, B, sr, 8, counts(5, 1), counts(0, 1))[0] == INVALID   # a range fault, then too few
    assert dec(S, 2, A, so, 8, B, sr, 8, counts(1, 0), counts(1, 2)) == few(1, 1)    # two short stripes: the first
    eng.synchronize()


def test_encode_device_batch(eng, dev):
    A, B, _, _ = dev

    def enc(s, n, a, so, b, sr):
        return call("rs16_encode_device_batch", eng.h, K, M, s, n, a, so, b, sr, None)

    assert enc(BAD_S, 0, A, K * S, B, M * S)[0] == SHARD_SIZE    # rate before nstripes == 0
    assert enc(BAD_S, 2, A + 8, 64, B, M * S)[0] == SHARD_SIZE   # ... and before stride and alignment
    assert enc(S, 0, A + 8, 64, None, 32)[0] == OK               # nstripes == 0 before every array fault
    assert enc(S, 2, A + 8, K * S, B, M * S)[0] == INVALID
    assert enc(S, BIG, A, K * S, B, M * S)[0] == INVALID
    eng.synchronize()


def test_prepare(eng, dev):
    A, B, fo, fr = dev
    scratch = DeviceArray(eng, 1024)  # (a valid decode writes its originals: not into the guarded rows)
    X, R = scratch.ptr, scratch.ptr + 512

    def prepare(s, o, r):
        return call("rs16_decode_prepare", eng.h, K, M, s, fo, fr, o, r, None)

    def prepared(a=X, b=R):
        return call("rs16_decode_device_prepared", eng.h, K, M, S, a, b, None)

    assert prepare(S, 3, 1)[0] == OK and prepared()[0] == OK and prepared()[0] == INVALID  # consumed once
    # a failed preparation of any kind leaves none behind, whatever was prepared before
    for s, o, r, want in [(BAD_S, 3, 1, (SHARD_SIZE, BAD_S, 0, 0)), (S, 5, 0, (INVALID, 0, 0, 0)),
                          (S, 0, 3, (INVALID, 0, 0, 0)), (S, 1, 1, few(1, 1)), (BAD_S, 1, 1, (SHARD_SIZE, BAD_S, 0, 0))]:
        assert prepare(S, 3, 1)[0] == OK
        assert prepare(s, o, r) == want
        assert prepared()[0] == INVALID, (s, o, r)
    # a misaligned array is refused and the preparation survives (every original received: no launch)
    assert prepare(S, 4, 0)[0] == OK
    assert prepared(A + 8, B)[0] == INVALID and prepared(A, B + 8)[0] == INVALID
    assert prepared(A, B)[0] == OK
    eng.synchronize()


def host_stripes(n):
    orig = (np.arange(n * K * S) * 29 % 253).astype(np.uint8).reshape(n, K, S)
    rec = (np.arange(n * M * S) * 31 % 247).astype(np.uint8).reshape(n, M, S)
    return orig, rec


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


SHORT = np.array([0x80, 0, 0, 0], np.uint8), np.array([0xFF, 0], np.uint8)     # 1 + 1 < 4
ALL = np.array([1, 2, 0x40, 0xFF], np.uint8), np.array([0, 0x80], np.uint8)  # nothing lost


def test_decode_host(eng):
    orig, rec = host_stripes(1)
    keep = orig.copy()

    def dec(s, flags, h_rec=hp(rec)):
        return call("rs16_decode_host", eng.h, K, M, s, hp(orig), hp(flags[0]), h_rec, hp(flags[1]), 0)

    assert dec(BAD_S, SHORT)[0] == SHARD_SIZE    # rate before NotEnoughShards
    assert dec(BAD_S, ALL)[0] == SHARD_SIZE      # ... and before nothing lost
    assert dec(S, SHORT) == few(1, 1)
    assert dec(S, ALL, None)[0] == OK            # nothing lost: no device work, the recovery array is never read
    assert np.array_equal(orig, keep)


def test_decode_host_batch(eng):
    orig, rec = host_stripes(2)
    keep = orig.copy()
    so, sr = K * S, M * S

    def flags(*per_stripe):
        fo = np.zeros((2, 8), np.uint8)
        fr = np.zeros((2, 8), np.uint8)
        for i, (o, r) in enumerate(per_stripe):
            fo[i, :K], fr[i, :M] = o, r
        return fo, fr

    def dec(s, n, f, o_stride=so, fo_stride=8, h_orig=hp(orig), h_rec=hp(rec)):
        return call("rs16_decode_host_batch", eng.h, K, M, s, n, h_orig, o_stride, hp(f[0]), fo_stride, h_rec, sr,
                    hp(f[1]), 8)

    short2 = np.array([0, 0, 2, 0], np.uint8), np.array([0, 0], np.uint8)  # 1 + 0 < 4
    assert dec(BAD_S, 0, flags(SHORT, ALL))[0] == SHARD_SIZE                     # rate before nstripes == 0
    assert dec(S, 0, flags(SHORT, ALL), 64, 3, None, None)[0] == OK              # nstripes == 0 before the rest
    assert dec(S, 2, flags(SHORT, ALL), o_stride=64)[0] == INVALID               # stride before NotEnoughShards
    assert dec(S, 2, flags(SHORT, ALL), fo_stride=3)[0] == INVALID
    assert dec(S, 2, flags(SHORT, ALL), h_rec=None)[0] == INVALID                # NULL before NotEnoughShards
    assert dec(S, 2, flags(ALL, ALL), o_stride=64)[0] == INVALID                 # ... and before nothing lost
    assert dec(S, 2, flags(ALL, SHORT)) == few(1, 1)                             # NotEnoughShards of a later stripe
    assert dec(S, 2, flags(SHORT, short2)) == few(1, 1)                          # two short stripes: the first
    assert dec(S, 2, flags(short2, SHORT)) == few(1, 0)
    assert dec(S, 2, flags(ALL, ALL))[0] == OK                                   # nothing lost: nothing moves
    assert np.array_equal(orig, keep)


def test_decode_host_multi(eng):
    orig, rec = host_stripes(1)
    keep = orig.copy()

    def dec(engines, n, s, flags, h_rec=hp(rec)):
        return call("rs16_decode_host_multi", engines, n, K, M, s, hp(orig), hp(flags[0]), h_rec, hp(flags[1]))

    one = (C.c_void_p * 1)(eng.h)
    hole = (C.c_void_p * 2)(eng.h, None)
    assert dec(None, 1, BAD_S, SHORT)[0] == INVALID      # a NULL engine (array) before rate
    assert dec(one, 0, BAD_S, SHORT)[0] == INVALID
    assert dec(hole, 2, BAD_S, SHORT)[0] == INVALID
    assert dec(hole, 2, S, SHORT)[0] == INVALID          # ... and before NotEnoughShards
    assert dec(one, 1, BAD_S, SHORT)[0] == SHARD_SIZE    # rate before NotEnoughShards
    assert dec(one, 1, BAD_S, ALL)[0] == SHARD_SIZE
    assert dec(one, 1, S, SHORT) == few(1, 1)
    assert dec(one, 1, S, ALL, None)[0] == OK            # nothing lost: no device work
    assert np.array_equal(orig, keep)
