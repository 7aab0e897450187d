"""Wide shards through the pass kernels, with the launcher's own choice of
address form (no diag flag anywhere in this file), byte for byte against the
oracle.

Shard data is independent in 64-byte column blocks (32 elements: low bytes,
then high bytes), so beyond 1024 rows the oracle runs on sampled column
blocks only: the device arrays are filled with a non-zero constant
(rs16_memset_device), seeded random bytes go into the sampled blocks of every
row (pitched copies, one per run of adjacent blocks; whole arrays are never
uploaded), and the same blocks are read back.  A misaddressed read then
fetches the constant or another sample, a misaddressed write leaves the
constant in place: either is a mismatch.  The sampled blocks, always the same
set: the first and last of the row, those on each side of byte offsets 32768
and 65536 (the zero page's wrap, `offL & 0x7FFF`, and its size), those on
each side of every slab boundary in the 8 blocks at the middle of the row
(slabs are 2, 4 or 8 blocks: 16, 32, 64 quads), and in part (b) those on each
side of the offset at which a 32-bit lane offset would wrap.

(a) every pass program at every tile size T the codec reaches, at 33,344-byte
shards (521 blocks = 4168 quads: a partial last slab at 16, 32 and 64 quads
per slab, rows wider than the zero page's wrap) -- wider than 2048 B, so
the 512 / 1024-row transforms leave the column codec by themselves -- and at
65,600 bytes (wider than the zero page).

(b) the launcher's predicate at its natural limits, at the smallest shape
that reaches them: a 4 GiB lane offset needs 2^11 rows of 8 MiB (below 16 GiB
no array holds one).  Engine.fft / ifft of 2^11 rows run a T = 6, lo = 5 pass
(two 16-row sets per wave: a lane's rows start up to 512 rows below its
wave's) and a T = 5, lo = 0 pass.  tests/test_pass_launch_consts.py is the
model of the same decisions on the CPU.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import PassConsts, RS16Error, lib
from rs16.device import DeviceArray, PinnedArray

gpu = pytest.mark.gpu

S_WIDE, S_PAGE = 33344, 65600
FILL_IN, FILL_OUT, FILL_LOST = 0x5A, 0x77, 0xA5
FULL_ROWS_MAX = 1024  # up to here whole rows go through the oracle


def sample_blocks(S, extra=()):
    nb = S // 64
    want = {0, nb - 1}
    for off in (32768, 65536):
        want |= {off // 64 - 1, off // 64}
    mid = nb // 2 // 8 * 8
    want |= set(range(mid - 1, mid + 9))
    want |= set(extra)
    return sorted(b for b in want if 0 <= b < nb)


def _check(rc, err):
    if rc:
        raise rs16.Error._from_c(err)


class Columns:
    """Chosen 64-byte column blocks of a rows x S device array <-> a host
    matrix of rows x (64 x blocks), through one pinned staging buffer."""

    def __init__(self, eng, rows, S, blocks):
        self.eng, self.rows, self.S, self.blocks = eng, rows, S, blocks
        self.width = 64 * len(blocks)
        self.stage = PinnedArray(eng, rows * self.width)
        # runs of adjacent blocks: (first block, column in the matrix, blocks)
        self.runs = []
        for i, b in enumerate(blocks):
            if self.runs and self.runs[-1][0] + self.runs[-1][2] == b:
                self.runs[-1][2] += 1
            else:
                self.runs.append([b, i, 1])

    def _copy(self, fn, d_ptr, to_device):
        err = RS16Error()
        for b, col, n in self.runs:
            dev, host = d_ptr + 64 * b, self.stage.ptr + 64 * col
            args = (dev, self.S, host, self.width) if to_device else (host, self.width, dev, self.S)
            _check(fn(self.eng.h, *args, 64 * n, self.rows, None, C.byref(err)), err)

    def put(self, d_ptr, m):
        assert m.shape == (self.rows, self.width)
        self.stage.array[:] = m.reshape(-1)
        self._copy(lib().rs16_memcpy2d_htod, d_ptr, True)

    def get(self, d_ptr):
        self.eng.synchronize()
        self.stage.array[:] = 0xEE  # (not what put() left there)
        self._copy(lib().rs16_memcpy2d_dtoh, d_ptr, False)
        return self.stage.array.reshape(self.rows, self.width).copy()


def fill(eng, d_ptr, value, nbytes):
    err = RS16Error()
    _check(lib().rs16_memset_device(eng.h, d_ptr, value, nbytes, None, C.byref(err)), err)


class Array:
    """A rows x S device array seen through its sampled blocks (or, up to
    FULL_ROWS_MAX rows, whole: every block is a sample)."""

    def __init__(self, eng, rows, S, value, blocks):
        self.eng, self.rows, self.S = eng, rows, S
        self.d = DeviceArray(eng, rows * S)
        self.cols = Columns(eng, rows, S, blocks)
        fill(eng, self.d.ptr, value, rows * S)

    @property
    def ptr(self):
        return self.d.ptr

    def put(self, m):
        self.cols.put(self.d.ptr, m)

    def get(self):
        return self.cols.get(self.d.ptr)


_cache = {}


def stripe(k, m, S, blocks):
    """(originals, the oracle's recovery) of the sampled blocks of a k:m x S
    stripe, computed once and read-only."""
    key = (k, m, S)
    if key not in _cache:
        w = 64 * len(blocks)
        orig = np.random.default_rng(k * 7 + m * 3 + S).integers(0, 256, (k, w), dtype=np.uint8)
        rec = O.encode(k, m, orig)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (orig, rec)
    return _cache[key]


def blocks_for(rows, S):
    return list(range(S // 64)) if rows <= FULL_ROWS_MAX else sample_blocks(S)


def flags(eng, a):
    return DeviceArray.from_numpy(eng, np.ascontiguousarray(a, np.uint8))


def run_codec(k, m, S, decodes=True):
    """Encode k:m x S; then (k = m) the decode with every original lost and
    the general decode of a seeded third of them."""
    eng = rs16.default_engine()
    blocks = blocks_for(max(k, m), S)
    orig, want = stripe(k, m, S, blocks)
    d_o = Array(eng, k, S, FILL_IN, blocks)
    d_r = Array(eng, m, S, FILL_OUT, blocks)
    d_o.put(orig)
    rs16.encode_device(k, m, S, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_r.get(), want), "encode"
    assert np.array_equal(d_o.get(), orig), "the originals stay"
    if not decodes:
        return
    # every original lost, recovery 0 .. k received (k >= 2048: the identity decode)
    d_o.put(np.full_like(orig, FILL_LOST))
    d_of, d_rf = flags(eng, np.zeros(k)), flags(eng, np.ones(m))
    rs16.decode_device(k, m, S, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, m, engine=eng, check=True)
    assert np.array_equal(d_o.get(), orig), "decode, every original lost"
    assert np.array_equal(d_r.get(), want), "the recovery stays"
    # a seeded third of the originals lost, as many seeded recovery shards received
    rng = np.random.default_rng(k + S)
    lost = rng.choice(k, max(1, k // 3), replace=False)
    of, rf = np.ones(k, np.uint8), np.zeros(m, np.uint8)
    of[lost] = 0
    rf[rng.choice(m, len(lost), replace=False)] = 1
    holes = orig.copy()
    holes[lost] = FILL_LOST
    d_o.put(holes)
    d_of, d_rf = flags(eng, of), flags(eng, rf)
    rs16.decode_device(k, m, S, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, k - len(lost), len(lost), engine=eng,
                       check=True)
    assert np.array_equal(d_o.get(), orig), "decode, a third of the originals lost"
    assert np.array_equal(d_r.get(), want), "the recovery stays"


def test_sampled_blocks():
    # (CPU) the sample set of the two widths and of an 8 MiB row
    b = sample_blocks(S_WIDE)
    assert b == [0, 255, 256, 257, 258, 259, 260, 261, 262, 263, 264, 511, 512, 520]
    b = sample_blocks(S_PAGE)
    assert {0, 511, 512, 1023, 1024} <= set(b) and set(range(511, 521)) <= set(b) and len(b) == 13
    b = sample_blocks(8388608, extra=(130559, 130560))
    assert {0, 511, 512, 1023, 1024, 65535, 65536, 65544, 130559, 130560, 131071} <= set(b)


@gpu
@pytest.mark.parametrize("j", list(range(1, 13)) + [14, 15])
def test_wide_rows(j):
    # j <= 8: the single-pass programs at T = j; 9 .. 15: three passes at
    # T = j // 2 and j - j // 2 (the decodes: of j + 1 row bits); 14, 15: the
    # wave-staged T = 7 / 8 encode passes
    run_codec(1 << j, 1 << j, S_WIDE)


@gpu
@pytest.mark.parametrize("k,m", [(20000, 20000), (300, 2000)])
def test_wide_rows_uneven(k, m):
    # zero-gathered rows and a partial last recovery tile; the low rate's
    # multi-chunk encode (one chunk of originals read by every recovery
    # chunk: in_rows_mask)
    run_codec(k, m, S_WIDE, decodes=False)


@gpu
@pytest.mark.parametrize("j", [9, 11])
def test_rows_wider_than_the_zero_page(j):
    run_codec(1 << j, 1 << j, S_PAGE)


# ---------------------------------------------------------------------------
# (b) the predicate's natural limits
# ---------------------------------------------------------------------------
ROWS_B, S_MAX_B = 2048, 8388608
T_HI, LO_HI, T_LO = 6, 5, 5  # Engine.fft / ifft of 2^11 rows: a T = 6, lo = 5 pass and a T = 5, lo = 0 pass


@functools.lru_cache(None)
def prog_id(name):
    return next(p for p in range(lib().rs16_prog_count()) if lib().rs16_prog_name(p) == name.encode())


def pass_consts(prog, T, lo, S):
    out = PassConsts()
    assert lib().rs16_host_pass_consts(prog_id(prog), T, lo, S, S, S, S, S // 8, 0, 0, 0, 0, C.byref(out))
    return out


def picked_widths():
    """Two multiples of 256 B picked through the hook, over the T = 6 passes
    of both transforms: the largest width with full_lanes = 1, and the
    smallest with voff32 = 1 and full_lanes = 0 where only rs_out causes it
    (the width is a multiple of the kernel's quads: 256 B)."""
    largest_full, smallest_rs = 0, None
    for S in range(256, S_MAX_B + 1, 256):
        for prog in ("GEN_FFT", "GEN_IFFT"):
            c = pass_consts(prog, T_HI, LO_HI, S)
            if c.full_lanes:
                largest_full = max(largest_full, S)
            elif c.voff32 and smallest_rs is None:
                smallest_rs = S
    return largest_full, smallest_rs


def lane_top(c, lo, S):
    """The model's largest lane offset of a full-width launch (layout A)."""
    return (((c.row_sets - 1) << c.reg_bits) << lo) * S + S - 4


def test_picked_widths():
    # (CPU) what the hook picks, against the model's arithmetic: the largest
    # full-lanes width is the last multiple of 256 whose T = 6 offsets fit
    # (513 S <= 2^32); the stores of GEN_IFFT, in layout B (row registers 2^2
    # tile rows apart), step by S << 7, which reaches 2^28 at S = 2^21
    assert picked_widths() == ((1 << 32) // 513 // 256 * 256, 1 << 21) == (8372224, 2097152)


@gpu
def test_predicate_limits():
    eng = rs16.default_engine()
    try:
        d = DeviceArray(eng, ROWS_B * S_MAX_B)
    except rs16.Error as e:
        if e.kind == "DeviceError" and e.fields.get("hip_error") == 2:  # hipErrorOutOfMemory
            pytest.skip(f"17.2 GB device allocation: {e}")
        raise
    full, rs_only = picked_widths()
    # width -> (voff32, full_lanes) of the T = 6, lo = 5 pass of (GEN_FFT, GEN_IFFT)
    cases = {
        8372288: ((0, 0), (0, 0)),  # 513 S - 4 >= 2^32: the first width whose lane offsets need 64 bits
        8388544: ((0, 0), (0, 0)),  # the last width below 2^23
        8388608: ((0, 0), (0, 0)),  # 512 S = 2^32
        full: ((1, 1), (1, 0)),     # GEN_IFFT: rs_out = S << 7 >= 2^28
        rs_only: ((1, 1), (1, 0)),
    }
    for S, expect in cases.items():
        wrap = (1 << 32) - (((2 - 1) << 4) << LO_HI) * S  # byte of the row at which a 32-bit lane offset would wrap
        blocks = sample_blocks(S, extra=(wrap // 64 - 1, wrap // 64) if 0 <= wrap < S else ())
        cols = Columns(eng, ROWS_B, S, blocks)
        for (prog, fn), (v32, fl) in zip((("GEN_FFT", eng.fft), ("GEN_IFFT", eng.ifft)), expect):
            hi, lo = pass_consts(prog, T_HI, LO_HI, S), pass_consts(prog, T_LO, 0, S)
            assert (hi.row_sets, hi.reg_bits, lo.row_sets, lo.reg_bits) == (2, 4, 4, 3)
            assert (hi.voff32, hi.full_lanes) == (v32, fl), (S, prog)
            assert bool(hi.voff32) == (lane_top(hi, LO_HI, S) < 1 << 32), (S, prog)  # the exact predicate
            assert lo.voff32 == 1 and lane_top(lo, 0, S) < 1 << 31, (S, prog)
            trunc = ROWS_B if prog == "GEN_FFT" else 2000
            x = np.random.default_rng(S + trunc).integers(0, 256, (ROWS_B, cols.width), dtype=np.uint8)
            x[trunc:] = 0  # IFFT contract: zero tail (whole rows, below)
            fill(eng, d.ptr, FILL_IN, ROWS_B * S)
            if trunc < ROWS_B:
                fill(eng, d.ptr + trunc * S, 0, (ROWS_B - trunc) * S)
            cols.put(d.ptr, x)
            fn(d.ptr, ROWS_B, S, 0, ROWS_B, trunc, 0)
            want = x.copy()
            (O.fft if prog == "GEN_FFT" else O.ifft)(want, 0, ROWS_B, trunc, 0)
            assert np.array_equal(cols.get(d.ptr), want), (S, prog)
