"""One small decode per (eval form x ErasureSpec feature) pair of the erasure
evaluation (rs16_eval.hip): the forms are eval_small_kernel<1|2|4|8>,
eval_fused_kernel and the two-kernel form (fwht_lo_flags_kernel +
fwht_hi_mulw_kernel), each with and without the closing fwht_lo_kernel
(last_lo); the features are the pass metadata (rbits, zflags, rcount), the lost
originals' row range of a pruned general decode, lost_all (the repair), wanted
(the selective decode, the read set at every address mod 4) and the strides
of a batch whose stripes have losses of their own.  Which form each case
reaches was read once from a host-side print in the launcher
(profiles/r23_eval_forms.txt).

Every case has 64-byte shards and an engine under DIAG_NO_COLUMN, so that the
pass codec and with it the evaluation run at these sizes.  Restored shards are
compared bit for bit with the originals the oracle's recovery shards were made
from (regenerated recovery shards with the oracle's), slots the call does not
restore must keep their bytes, and the single-pattern calls run with
check=True (the received counts, from rcount).
"""
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16.device import DeviceArray
from rs16.util import generate_original

pytestmark = pytest.mark.gpu

SB = 64
FULL, TWO = rs16.DIAG_EVAL_FULL, rs16.DIAG_EVAL_TWO_KERNEL


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    e.set_diagnostics(rs16.DIAG_NO_COLUMN)
    e.set_profiling(True)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, seed=0):
    """(originals, oracle recovery) of one stripe, computed once, read-only."""
    original = generate_original(k, SB, 31 * k + m + seed)
    recovery = O.encode(k, m, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def scattered(k, m, seed=0):
    """Received masks with about a third of the possible losses, scattered, and
    two recovery shards more than needed."""
    rng = np.random.default_rng(1000 * k + m + seed)
    nl = max(2, min(k, m) // 3)
    om, rm = np.ones(k, bool), np.zeros(m, bool)
    om[rng.choice(k, nl, replace=False)] = False
    rm[rng.choice(m, min(m, nl + 2), replace=False)] = True
    return om, rm


def all_lost(k, m):
    return np.zeros(k, bool), np.ones(m, bool)


def flag_array(eng, mask, off=0):
    """The flag bytes of mask (rows of a 2-D mask = stripes) on the device,
    off bytes past an aligned address: (array, pointer)."""
    d = DeviceArray.from_numpy(eng, np.concatenate([np.full(off, 7, np.uint8), mask.astype(np.uint8).ravel()]))
    return d, d.ptr + off


def decode(eng, k, m, om, rm, diag=0, how="decode", flag_off=0, wanted=None, wanted_off=0):
    """One single-pattern call on a stripe with the rows outside om / rm
    overwritten, checked as the module's docstring says."""
    original, recovery = stripe(k, m)
    held, rec = original.copy(), recovery.copy()
    held[~om] = 0xA5
    rec[~rm] = 0x5A
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, rec)
    d_fo, p_fo = flag_array(eng, om, flag_off)
    d_fr, p_fr = flag_array(eng, rm, flag_off)
    no, nr = int(om.sum()), int(rm.sum())
    want_o, want_r = original.copy(), rec
    old = eng.set_diagnostics(rs16.DIAG_NO_COLUMN | diag)
    try:
        eng.profile_reset()
        if how == "decode":
            rs16.decode_device(k, m, SB, d_o.ptr, p_fo, d_r.ptr, p_fr, no, nr, engine=eng, check=True)
        elif how == "repair":
            rs16.repair_device(k, m, SB, d_o.ptr, p_fo, d_r.ptr, p_fr, no, nr, engine=eng, check=True)
            want_r = recovery
        else:
            d_w, p_w = flag_array(eng, wanted, wanted_off)
            rs16.decode_device_select(k, m, SB, d_o.ptr, p_fo, p_w, d_r.ptr, p_fr, no, nr, int((wanted & ~om).sum()),
                                      engine=eng, check=True)
            want_o[~om & ~wanted] = 0xA5
        got_o, got_r = d_o.download(shape=(k, SB)), d_r.download(shape=(m, SB))
        ran = {n: c for n, (_, c) in eng.profile().items() if c}
    finally:
        eng.set_diagnostics(old)
    assert ran.get("EVAL_POLY") == 1, ran
    assert np.array_equal(got_o, want_o)
    assert np.array_equal(got_r, want_r)


# ---- the small form, eval_small_kernel<NB>: the high rate with n = 256 NB rows ----
@pytest.mark.parametrize("nb,k,m", [(1, 100, 100), (2, 300, 100), (4, 600, 200), (8, 1200, 500)],
                         ids=["small1", "small2", "small4", "small8"])
def test_small_general(eng, nb, k, m):
    decode(eng, k, m, *scattered(k, m))


def test_small_last_lo(eng):
    # every original lost: the one-pass half decode of 256-row halves, whose
    # erasure logs the closing fwht_lo_kernel finishes
    decode(eng, 256, 256, *all_lost(256, 256))


# ---- the fused form: segments on 256-row blocks, n = 1024 ----
def test_fused_low_rate(eng):
    decode(eng, 256, 512, *scattered(256, 512))


def test_fused_high_rate(eng):
    decode(eng, 512, 256, *scattered(512, 256), diag=FULL)


def test_fused_last_lo(eng):
    decode(eng, 256, 256, *all_lost(256, 256), diag=FULL)


# ---- the two-kernel form: by its switch, and by flag arrays at odd addresses ----
@pytest.mark.parametrize("why", ["switch", "odd_flags"])
def test_two_kernel_low_rate(eng, why):
    decode(eng, 256, 512, *scattered(256, 512), diag=TWO if why == "switch" else 0,
           flag_off=int(why == "odd_flags"))


@pytest.mark.parametrize("why", ["switch", "odd_flags"])
def test_two_kernel_high_rate(eng, why):
    decode(eng, 512, 256, *scattered(512, 256), diag=FULL | (TWO if why == "switch" else 0),
           flag_off=int(why == "odd_flags"))


@pytest.mark.parametrize("why", ["switch", "odd_flags"])
def test_two_kernel_last_lo(eng, why):
    decode(eng, 256, 256, *all_lost(256, 256), diag=FULL | (TWO if why == "switch" else 0),
           flag_off=int(why == "odd_flags"))


# ---- wanted: the fused form assembles the read set's first and last dword of
# a block by hand when the read set is not dword-aligned ----
def select_masks(k, m):
    om, rm = scattered(k, m, seed=5)
    om[[0, 1, 255, 256, k - 2, k - 1]] = False  # the ends of both 256-row blocks of originals
    rm[:] = False
    rm[:int((~om).sum()) + 2] = True
    wanted = np.zeros(k, bool)
    wanted[np.flatnonzero(~om)[::2]] = True     # every second lost original ...
    wanted[[0, k - 1]] = True                   # ... the first and the last original among them
    wanted[np.flatnonzero(om)[::7]] = True      # and some received ones
    return om, rm, wanted


@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_select_fused(eng, off):
    k, m = 512, 256
    om, rm, wanted = select_masks(k, m)
    decode(eng, k, m, om, rm, diag=FULL, how="select", wanted=wanted, wanted_off=off)


def test_select_small(eng):
    k, m = 600, 200
    om, rm, wanted = select_masks(k, m)
    decode(eng, k, m, om, rm, how="select", wanted=wanted, wanted_off=1)


def test_select_two_kernel(eng):
    k, m = 512, 256
    om, rm, wanted = select_masks(k, m)
    decode(eng, k, m, om, rm, diag=FULL | TWO, how="select", wanted=wanted, wanted_off=3)


# ---- lost_all: a lost recovery shard and a lost original in different 256-row blocks ----
def repair_masks(k, m, lost_original, lost_recovery):
    om, rm = np.ones(k, bool), np.ones(m, bool)
    om[lost_original] = False
    rm[lost_recovery] = False
    return om, rm


def test_repair_fused(eng):
    decode(eng, 512, 256, *repair_masks(512, 256, 300, 3), diag=FULL, how="repair")  # rows 3 and 556


def test_repair_small(eng):
    decode(eng, 600, 200, *repair_masks(600, 200, 400, 3), how="repair")  # rows 3 and 656


def test_repair_two_kernel(eng):
    decode(eng, 512, 256, *repair_masks(512, 256, 300, 3), diag=FULL | TWO, how="repair")


# ---- a batch whose stripes have losses of their own ----
@pytest.mark.parametrize("form,k,m,pad", [("fused", 256, 512, 0), ("two_kernel", 256, 512, 1), ("small", 600, 200, 0)])
def test_varied_batch(eng, form, k, m, pad):
    """Two stripes with different losses; pad = bytes between the stripes'
    flag arrays (a stride that is no multiple of 16 rules the fused form out)."""
    ns = 2
    stripes = [stripe(k, m, seed=i) for i in range(ns)]
    masks = [scattered(k, m, seed=i) for i in range(ns)]
    om, rm = np.stack([a for a, _ in masks]), np.stack([b for _, b in masks])
    original = np.stack([o for o, _ in stripes])
    held, rec = original.copy(), np.stack([r for _, r in stripes])
    held[~om] = 0xA5
    rec[~rm] = 0x5A
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, rec)
    fo = np.concatenate([om.astype(np.uint8), np.full((ns, pad), 7, np.uint8)], axis=1)
    fr = np.concatenate([rm.astype(np.uint8), np.full((ns, pad), 7, np.uint8)], axis=1)
    d_fo, d_fr = DeviceArray.from_numpy(eng, fo), DeviceArray.from_numpy(eng, fr)
    eng.profile_reset()
    rs16.decode_device_batch_varied(k, m, SB, ns, d_o.ptr, k * SB, d_fo.ptr, k + pad, d_r.ptr, m * SB, d_fr.ptr,
                                    m + pad, om.sum(1), rm.sum(1), engine=eng)
    got_o, got_r = d_o.download(shape=(ns, k, SB)), d_r.download(shape=(ns, m, SB))
    ran = {n: c for n, (_, c) in eng.profile().items() if c}
    assert ran.get("EVAL_POLY") == 1, ran
    assert np.array_equal(got_o, original)
    assert np.array_equal(got_r, rec)
