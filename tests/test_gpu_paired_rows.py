"""Paired rows of the work buffer (rs16_pass.hpp
pass_kernel_late_paired): between the three passes of an encode or of an
identity decode the engine may keep a quad's low and high dword next to each
other in its work buffer Z, so that a lane moves a row with one 8-byte access.
The form is a property of the sequence -- the pass that writes Z and the pass
that reads it must agree -- and one host function decides it
(z_form_sequence, shown here as rs16_host_paired_rows): paired exactly
when all three launches report late_rows and full_lanes and
RS16_DIAG_NO_PAIRED_ROWS is not set.  Results are the same bits either way.

Every GPU case is bit-exact against the oracle at the smallest stripes whose
three passes are late-rows kernels (2^14 rows: T = 7 / 7 / 7; 2^15 rows: T =
7 / 8 / 7) and at the smallest width with full lanes (512 B: one slab of 64
quads at T = 7, two of 32 at T = 8), and asserts through the hook which side
of the switch its sequences take.  (The non-identity half decode and the
general decode never ask the hook: their launches are unpaired by
construction, and what those cases assert is the bits -- their ENC_MID runs
on rows a decoder pass wrote.)

The CPU case compares the hook with its definition, the AND over the three
launches' late_rows & full_lanes from rs16_host_pass_consts_rows, over chunk
sizes, widths (also those around the 2^28 row-register stride bound and the
2^32 lane-offset bound, which no device array of a test reaches) and row
limits around wave and tile boundaries."""
import ctypes as C

import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import PassConsts, lib
from rs16.device import DeviceArray
from rs16.util import generate_original

gpu = pytest.mark.gpu

_cache = {}


def _stripe(k, m, sb, seed=0):
    """(originals, the oracle's recovery) of a k:m x sb stripe, computed once."""
    key = (k, m, sb, seed)
    if key not in _cache:
        orig = generate_original(k, sb, k + m + sb + seed)
        rec = O.encode(k, m, orig)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (orig, rec)
    return _cache[key]


# ---------------------------------------------------------------------------
# The hook, and its definition from the three launches.
# ---------------------------------------------------------------------------
_progs = {}


def _prog(name):
    if not _progs:
        _progs.update({lib().rs16_prog_name(i).decode(): i for i in range(lib().rs16_prog_count())})
    return _progs[name]


def _paired(chunk, sb, a_count, diag=0, s_user=None, seg_chunk=0, row_base_in=0):
    return lib().rs16_host_paired_rows(chunk, sb, sb if s_user is None else s_user, a_count, seg_chunk, row_base_in,
                                       diag)


def _chunk(m):
    return 1 << (m - 1).bit_length()


def _encode_paired(k, m, sb, diag=0, s_user=None):
    return _paired(_chunk(m), sb, k, diag, s_user)


def _decode_paired(k, sb, diag=0):
    # the identity decode of k:k: the received half (k rows) through the
    # encoder's passes, with the decode's segment boundary k and the half's
    # first work row (0 or k by the rate) in the launch arguments
    got = {_paired(k, sb, k, diag, seg_chunk=k, row_base_in=base) for base in (0, k)}
    assert len(got) == 1
    return got.pop()


def _launch(prog, T, lo, s_in, s_out, s_seg, qrow, chunk, row_base_in, a_count, diag):
    out = PassConsts()
    assert lib().rs16_host_pass_consts_rows(_prog(prog), T, lo, s_in, s_out, s_seg, s_in, qrow, chunk, row_base_in, 0,
                                            a_count, diag, C.byref(out))
    return out


def _definition(chunk, sb, s_user, a_count, seg_chunk, row_base_in, diag):
    """The three launches as the engine plans them (rs16_engine.cpp
    encode_high_fused): L / 2 contiguous row bits gathered from the caller's
    rows, L - L / 2 strided ones on Z, L / 2 contiguous ones stored to the
    caller's rows."""
    if diag & rs16.DIAG_NO_PAIRED_ROWS:
        return 0
    L = chunk.bit_length() - 1
    lo, hi = L // 2, L - L // 2
    ok = 1
    for prog, T, l, s_out in (("ENC_FIRST", lo, 0, sb), ("ENC_MID", hi, lo, sb), ("ENC_LAST", lo, 0, s_user)):
        c = _launch(prog, T, l, sb, s_out, s_user, sb // 8, seg_chunk, row_base_in, a_count, diag)
        ok &= c.late_rows & c.full_lanes
    return ok


# ---------------------------------------------------------------------------
# GPU cases
# ---------------------------------------------------------------------------
def _encode(eng, k, m, sb):
    orig, want = _stripe(k, m, sb)
    d_o = DeviceArray.from_numpy(eng, orig)
    d_r = DeviceArray.from_numpy(eng, np.full(m * sb, 0x77, np.uint8))
    rs16.encode_device(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    assert np.array_equal(d_r.download(shape=(m, sb)), want)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)  # the originals stay


def _identity_decode(eng, k, sb, check):
    # every original lost, recovery 0 .. k received; check=True has the first
    # and last pass count the received flags and compares the counts
    orig, rec = _stripe(k, k, sb)
    d_o = DeviceArray.from_numpy(eng, np.full(k * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(k, np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, k, engine=eng, check=check)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)
    assert np.array_equal(d_r.download(shape=(k, sb)), rec)  # the recovery stays


def _general_decode(eng, k, sb, nlost, seed):
    # nlost scattered originals lost, as many scattered recovery shards received
    orig, rec = _stripe(k, k, sb)
    rng = np.random.default_rng(seed)
    om = np.ones(k, bool)
    om[rng.choice(k, nlost, replace=False)] = False
    rm = np.zeros(k, bool)
    rm[rng.choice(k, nlost, replace=False)] = True
    held = orig.copy()
    held[~om] = 0xA5
    d_o = DeviceArray.from_numpy(eng, held)
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, om.astype(np.uint8))
    d_rf = DeviceArray.from_numpy(eng, rm.astype(np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, int(om.sum()), nlost, engine=eng, check=True)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)


@gpu
@pytest.mark.parametrize("n,sb", [(16384, 512), (32768, 512), (32768, 1024)])
def test_encode(n, sb):
    assert _encode_paired(n, n, sb) == 1
    _encode(rs16.default_engine(), n, n, sb)


@gpu
def test_encode_zero_page_waves():
    # the row limit 24576 = 192 x 128 is aligned: the gather's waves above it
    # read the zero page and write paired rows of zeros
    assert _encode_paired(24576, 32768, 512) == 1
    _encode(rs16.default_engine(), 24576, 32768, 512)


@gpu
def test_encode_limit_between_two_waves():
    # 20000 = 156 x 128 + 32 = 1250 x 16: the limit lies between two waves of
    # a tile -- direct and zero-page waves in one workgroup, all storing pairs
    assert _encode_paired(20000, 20000, 512) == 1
    _encode(rs16.default_engine(), 20000, 20000, 512)


@gpu
def test_encode_first_pass_not_late():
    # 19992 = 1249 x 16 + 8 cuts a wave: the first pass keeps pass_kernel, so
    # the whole sequence is unpaired although the other two passes qualify
    assert rs16.use_high_rate(19992, 20000)  # (the fused three-pass encoder)
    chunk, sb = 32768, 512
    first = _launch("ENC_FIRST", 7, 0, sb, sb, sb, sb // 8, 0, 0, 19992, 0)
    mid = _launch("ENC_MID", 8, 7, sb, sb, sb, sb // 8, 0, 0, 19992, 0)
    last = _launch("ENC_LAST", 7, 0, sb, sb, sb, sb // 8, 0, 0, 19992, 0)
    assert [(c.late_rows, c.full_lanes) for c in (first, mid, last)] == [(0, 1), (1, 1), (1, 1)]
    assert _paired(chunk, sb, 19992) == 0
    _encode(rs16.default_engine(), 19992, 20000, sb)


@gpu
@pytest.mark.parametrize("sb", [64, 1088])
def test_encode_partial_slabs_unpaired(sb):
    # widths that are no multiple of 512 B have lanes without a quad
    # (full_lanes 0): late rows, but the reference form in Z
    assert _encode_paired(16384, 16384, sb) == 0
    _encode(rs16.default_engine(), 16384, 16384, sb)


@gpu
@pytest.mark.parametrize("check", [False, True], ids=["plain", "check"])
@pytest.mark.parametrize("k", [16384, 32768])
def test_identity_decode(k, check):
    assert _decode_paired(k, 512) == 1
    _identity_decode(rs16.default_engine(), k, 512, check)


@gpu
@pytest.mark.parametrize("k", [16384, 32768])
def test_half_decode_without_identity(k):
    # DEC_FIRST -> ENC_MID -> DEC_HALF_LAST: the same ENC_MID kernels, on rows
    # a decoder pass wrote in the reference form -- launched unpaired
    eng = rs16.Engine(0)
    eng.set_diagnostics(rs16.DIAG_NO_IDENTITY)
    _identity_decode(eng, k, 512, True)


@gpu
def test_forms_alternate_on_one_engine():
    # Z keeps whatever the last sequence left in it, in that sequence's form:
    # every sequence writes all it reads, so stale rows of the other form
    # must not matter
    eng = rs16.Engine(0)
    k, sb = 16384, 512
    assert _encode_paired(k, k, sb) == 1 and _decode_paired(k, sb) == 1 and _encode_paired(k, k, 64) == 0
    _encode(eng, k, k, sb)                         # paired
    _general_decode(eng, k, sb, k // 100, seed=5)  # DEC_FIRST / DEC_MID / DEC_LAST, unpaired
    _identity_decode(eng, k, sb, True)             # paired
    _encode(eng, k, k, 64)                         # unpaired
    _encode(eng, k, k, sb)                         # paired


@gpu
def test_two_batched_stripes():
    eng = rs16.default_engine()
    k = m = 16384
    sb, n, pad = 512, 2, 64
    assert _encode_paired(k, m, sb) == 1  # (per stripe: one geometry)
    so, sr = k * sb + pad, m * sb + pad
    pairs = [_stripe(k, m, sb), _stripe(k, m, sb, seed=1)]
    host_o = np.full(n * so, 0xEE, np.uint8)
    for i, (o, _) in enumerate(pairs):
        host_o[i * so:i * so + k * sb] = o.reshape(-1)
    d_o = DeviceArray.from_numpy(eng, host_o)
    d_r = DeviceArray.from_numpy(eng, np.full(n * sr, 0x77, np.uint8))
    rs16.encode_device_batch(k, m, sb, n, d_o.ptr, so, d_r.ptr, sr, engine=eng)
    got = d_r.download(shape=(n * sr,))
    for i, (_, rec) in enumerate(pairs):
        assert np.array_equal(got[i * sr:i * sr + m * sb].reshape(m, sb), rec), i
        assert (got[i * sr + m * sb:(i + 1) * sr] == 0x77).all(), i
    assert np.array_equal(d_o.download(shape=(n * so,)), host_o)  # originals and their padding stay


@gpu
def test_two_column_slices():
    # two 512 B slices of a 1024 B stripe: the caller's row stride is wider
    # than the slice, Z's is the slice width
    eng = rs16.Engine(0)
    eng.set_slices(2)
    k = m = 16384
    assert _encode_paired(k, m, 512, s_user=1024) == 1
    _encode(eng, k, m, 1024)
    assert _paired(k, 512, k, s_user=1024, seg_chunk=k, row_base_in=0) == 1
    _identity_decode(eng, k, 1024, True)


@gpu
@pytest.mark.parametrize("diag,paired", [("DIAG_NO_PAIRED_ROWS", 0), ("DIAG_NO_LATE_ROWS", 0), ("DIAG_FORCE_VOFF64", 0),
                                         ("DIAG_WIDE_TWIDDLES", 1)])
def test_diagnostics(diag, paired):
    # (DIAG_WIDE_TWIDDLES: paired, through the 12-lookup middle kernels)
    flag = getattr(rs16, diag)
    assert _encode_paired(32768, 32768, 512, flag) == paired
    assert _decode_paired(16384, 512, flag) == paired
    eng = rs16.Engine(0)
    eng.set_diagnostics(flag)
    _encode(eng, 32768, 32768, 512)
    _identity_decode(eng, 16384, 512, True)


# ---------------------------------------------------------------------------
# CPU: the hook against its definition.
# ---------------------------------------------------------------------------
def _row_limits(chunk):
    """Row limits around the wave (16 rows) and tile boundaries of the first pass."""
    L = chunk.bit_length() - 1
    tile = 1 << (L // 2)
    cand = {0, 1, 15, 16, 17, chunk - 16, chunk - 1, chunk}
    for j in (1, 2, 3, chunk // tile // 2, chunk // tile - 1):
        for d in (-16, -8, -1, 0, 1, 8, 16):
            cand.add(j * tile + d)
    return sorted(c for c in cand if 0 <= c <= chunk)


def test_hook_matches_definition():
    # widths: every multiple of 64 up to 4096; around 2^21, where the strided
    # pass's row-register stride S << 7 reaches 2^28 and, at T = 8 (two row
    # sets per wave, 2048 rows apart), the lane offset 2048 S + S reaches 2^32
    widths = list(range(64, 4096 + 64, 64)) + [(1 << 21) + d for d in (-2048, -1536, -1024, -512, 0, 512)]
    seen = set()
    for L in range(11, 16):
        chunk = 1 << L
        limits = _row_limits(chunk)
        for sb in widths:
            wide = sb > 4096
            for s_user in (sb, 2 * sb):
                for a_count in (limits if not wide else (chunk,)):
                    for seg_chunk, base in ((0, 0), (chunk, chunk)):
                        for diag in (0, rs16.DIAG_NO_PAIRED_ROWS) if a_count == chunk else (0,):
                            want = _definition(chunk, sb, s_user, a_count, seg_chunk, base, diag)
                            got = _paired(chunk, sb, a_count, diag, s_user, seg_chunk, base)
                            assert got == want, (chunk, sb, s_user, a_count, seg_chunk, base, diag)
                            seen.add((L, sb % 512 == 0, wide, got))
    # the sweep saw both sides where both exist, and one side where only one does
    for L in (11, 12, 13):
        assert not any(s[0] == L and s[3] for s in seen)
    for L in (14, 15):
        assert (L, True, False, 1) in seen and (L, True, False, 0) in seen
        assert (L, False, False, 1) not in seen
        assert (L, True, True, 1) in seen and (L, True, True, 0) in seen
