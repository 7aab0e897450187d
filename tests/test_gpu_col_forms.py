"""One small case per launched instantiation of the column codec (rs16_col.hip):
col_kernel<L, mode>, col2_kernel<L, mode> and colm_kernel<high>, 46 in all.
Every case has 64-byte shards (8 workgroups), is checked bit for bit against
the oracle -- a selective decode also that the lost originals outside the read
set keep their bytes -- and checks through Engine.profile() that the column
program ran and no pass program did.  Which instantiation each case reaches
was read once from a host-side print in the launchers
(profiles/r22_col_forms.txt).

The radix-4 kernel above 2^7 rows runs under DIAG_COL_RADIX4, except its
COL_DEC_EWORK forms (the low-rate Rate API decoders).
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
# (encode and all-lost half decode, general decode) per L = log2(rows of the transform)
ENC_SHAPE = {6: (50, 60), 7: (100, 100), 8: (200, 256), 9: (257, 512), 10: (600, 1024)}
GEN_SHAPE = {6: (20, 30), 7: (50, 60), 8: (100, 100), 9: (200, 256), 10: (300, 300), 11: (1000, 1000)}
EWORK_SHAPE = {9: (500, 512), 10: (1000, 1024)}                  # low-rate Rate API decoders
CHUNKS_HIGH = {8: (600, 256), 9: (1025, 512), 10: (2049, 1024)}  # COL_ENC_IFFT + COL_ENC_FFTX
CHUNKS_LOW = {8: (256, 600), 9: (512, 1025), 10: (1024, 2049)}   # COL_ENC, one grid row per chunk


def _cases():
    out = []
    for L in range(6, 11):
        for mode in ("ENC", "DEC_EVAL", "DEC_GEN", "DEC_GEN_SEL"):
            out.append(("col", L, mode, (GEN_SHAPE if "GEN" in mode else ENC_SHAPE)[L], L >= 8))
    for L in (9, 10):
        out.append(("col", L, "DEC_EWORK", EWORK_SHAPE[L], False))
    for mode in ("DEC_GEN", "DEC_GEN_SEL"):
        out.append(("col", 11, mode, GEN_SHAPE[11], True))
    for L in range(8, 11):
        for mode in ("ENC", "DEC_EVAL", "DEC_GEN", "DEC_GEN_SEL"):
            out.append(("col2", L, mode, (GEN_SHAPE if "GEN" in mode else ENC_SHAPE)[L], False))
        out.append(("col2", L, "ENC_IFFT", CHUNKS_HIGH[L], False))
        out.append(("col2", L, "ENC_FFTX", CHUNKS_HIGH[L], False))
    # (col2_kernel<L, ENC> is also the low rate's chunked encode: run with the ENC rows below)
    for mode in ("DEC_GEN", "DEC_GEN_SEL"):
        out.append(("col2", 11, mode, GEN_SHAPE[11], False))
    out.append(("colm", 7, "high", (129, 100), False))
    out.append(("colm", 7, "low", (100, 129), False))
    return out


CASES = _cases()
assert len(CASES) == 46


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    e.set_profiling(True)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, rate="default"):
    """(originals, oracle recovery) of one stripe, computed once, read-only."""
    original = generate_original(k, SB, 17 * k + m)
    recovery = O.encode(k, m, original) if rate == "default" else O.encode(k, m, original, rate=rate)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def launches(eng):
    return {n: c for n, (_, c) in eng.profile().items() if c}


def run_encode(eng, k, m, want_launches):
    original, want = stripe(k, m)
    d_o = DeviceArray.from_numpy(eng, original)
    d_r = DeviceArray.from_numpy(eng, np.full((m, SB), 0x5A, np.uint8))
    eng.profile_reset()
    rs16.encode_device(k, m, SB, d_o.ptr, d_r.ptr, engine=eng)
    got = d_r.download(shape=(m, SB))
    assert launches(eng) == {"COL_ENC": want_launches}, launches(eng)
    assert np.array_equal(got, want)


def run_decode(eng, k, m, lost, select):
    """Originals `lost` lost, as many recovery shards received (the first
    ones); select: every second lost original wanted, the others keep their
    bytes."""
    original, recovery = stripe(k, m)
    om, rm = np.ones(k, bool), np.zeros(m, bool)
    om[lost] = False
    rm[:len(lost)] = True
    held = original.copy()
    held[~om] = 0xA5
    rec = recovery.copy()
    rec[~rm] = 0x5A
    d_o, d_r = DeviceArray.from_numpy(eng, held), DeviceArray.from_numpy(eng, rec)
    d_fo = DeviceArray.from_numpy(eng, om.astype(np.uint8))
    d_fr = DeviceArray.from_numpy(eng, rm.astype(np.uint8))
    want = original.copy()
    eng.profile_reset()
    if select:
        wanted = np.zeros(k, np.uint8)
        wanted[np.asarray(lost)[::2]] = 1
        want[(~om) & (wanted == 0)] = 0xA5
        d_w = DeviceArray.from_numpy(eng, wanted)
        rs16.decode_device_select(k, m, SB, d_o.ptr, d_fo.ptr, d_w.ptr, d_r.ptr, d_fr.ptr, int(om.sum()),
                                  int(rm.sum()), int(wanted.sum()), engine=eng, check=True)
        prog = "COL_DEC_SEL"
    else:
        rs16.decode_device(k, m, SB, d_o.ptr, d_fo.ptr, d_r.ptr, d_fr.ptr, int(om.sum()), int(rm.sum()), engine=eng,
                           check=True)
        prog = "COL_DEC"
    got = d_o.download(shape=(k, SB))
    assert launches(eng) == {prog: 1}, launches(eng)
    assert np.array_equal(got, want)
    assert np.array_equal(d_r.download(shape=(m, SB)), rec), "recovery shards written"


def run_rate_decoder(eng, k, m):
    """The low-rate Rate API decoder, every original lost: eval_poly's kernel
    writes the engine's work logs, the column decoder finishes them."""
    original, recovery = stripe(k, m, "low")
    dec = rs16.RateDecoder(k, m, SB, rate="low", engine=eng)
    for i in range(k):
        dec.add_recovery_shard(i, recovery[i])
    eng.profile_reset()
    with dec.decode() as res:
        got = np.stack([np.frombuffer(res.restored_original(i), np.uint8) for i in range(k)])
    ran = launches(eng)
    assert ran == {"EVAL_POLY": 1, "COL_DEC": 1}, ran
    assert np.array_equal(got, original)


@pytest.mark.parametrize("kernel,L,mode,shape,radix4", CASES,
                         ids=["%s-L%d-%s" % (c[0], c[1], c[2]) for c in CASES])
def test_col_form(eng, kernel, L, mode, shape, radix4):
    k, m = shape
    old = eng.set_diagnostics(rs16.DIAG_COL_RADIX4 if radix4 else 0)
    try:
        if mode in ("ENC", "high", "low"):
            run_encode(eng, k, m, 1)
            if kernel == "col2" and mode == "ENC":  # the same instantiation, one grid row per chunk
                run_encode(eng, *CHUNKS_LOW[L], 1)
        elif mode in ("ENC_IFFT", "ENC_FFTX"):
            run_encode(eng, k, m, 2)  # (the chunks' IFFTs, then the FFT of their XOR)
        elif mode == "DEC_EVAL":
            run_decode(eng, k, m, list(range(k)), False)
        elif mode == "DEC_EWORK":
            run_rate_decoder(eng, k, m)
        else:
            # two lost originals in different 128-row blocks (the first and the last)
            run_decode(eng, k, m, [0, k - 1], mode == "DEC_GEN_SEL")
    finally:
        eng.set_diagnostics(old)
