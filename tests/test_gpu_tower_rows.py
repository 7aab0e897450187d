"""Tower form of the paired work rows on the device (DESIGN.md section 3.1;
rs16_pass.hpp pass_kernel_late_tower): the first pass writes Z's rows as a + b
beta over the GF(2^8) subfield, the middle pass works in that form (6-lookup
multiplies in its subfield layers) and the last pass converts back.  The form
never leaves the engine: recovery and restored shards are the same bits with
and without RS16_DIAG_NO_TOWER_ROWS, and equal the oracle's.

Shapes: the smallest stripes whose three passes are the paired kernels --
16384:16384 (T = 7 / 7 / 7, every middle layer a subfield layer) and
32768:32768 (7 / 8 / 7, one wide layer per direction) -- at 512 B (one slab of
the T = 7 passes) and 1024 B (two).  Every case asserts through the host
hooks which form its sequences take.  The oracle's results are computed once
per stripe and shared."""
import numpy as np
import pytest

import oracle_bind as O
import rs16
from rs16._lib import lib
from rs16.device import DeviceArray
from rs16.util import generate_original

gpu = pytest.mark.gpu

FORMS = [pytest.param(0, id="tower"), pytest.param(rs16.DIAG_NO_TOWER_ROWS, id="no_tower")]
SHAPES = [(16384, 512), (16384, 1024), (32768, 512), (32768, 1024)]

_cache = {}


def _stripe(k, m, sb, orig=None, key=None):
    key = key or (k, m, sb)
    if key not in _cache:
        if orig is None:
            orig = generate_original(k, sb, 7 * k + m + sb)
        rec = O.encode(k, m, orig)
        orig.setflags(write=False)
        rec.setflags(write=False)
        _cache[key] = (orig, rec)
    return _cache[key]


def _chunk(m):
    return 1 << (m - 1).bit_length()


def _forms(chunk, sb, a_count, diag, seg_chunk=0, base=0):
    L = lib()
    return (L.rs16_host_paired_rows(chunk, sb, sb, a_count, seg_chunk, base, diag),
            L.rs16_host_tower_rows(chunk, sb, sb, a_count, seg_chunk, base, diag))


def _engine(diag):
    eng = rs16.Engine(0)
    eng.set_diagnostics(diag)
    return eng


def _encode(eng, k, m, sb, orig, want):
    d_o = DeviceArray.from_numpy(eng, orig)
    d_r = DeviceArray.from_numpy(eng, np.full(m * sb, 0x77, np.uint8))
    rs16.encode_device(k, m, sb, d_o.ptr, d_r.ptr, engine=eng)
    return d_r.download(shape=(m, sb))


@gpu
@pytest.mark.parametrize("diag", FORMS)
@pytest.mark.parametrize("n,sb", SHAPES)
def test_encode(n, sb, diag):
    assert _forms(n, sb, n, diag) == (1, 0 if diag else 1)
    orig, want = _stripe(n, n, sb)
    assert np.array_equal(_encode(_engine(diag), n, n, sb, orig, want), want)


@gpu
@pytest.mark.parametrize("diag", FORMS)
@pytest.mark.parametrize("k,sb", SHAPES)
def test_identity_decode(k, sb, diag):
    # every original lost, recovery 0 .. k received: the encoder's three passes on the received half
    for base in (0, k):
        assert _forms(k, sb, k, diag, seg_chunk=k, base=base) == (1, 0 if diag else 1)
    orig, rec = _stripe(k, k, sb)
    eng = _engine(diag)
    d_o = DeviceArray.from_numpy(eng, np.full(k * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, rec)
    d_of = DeviceArray.from_numpy(eng, np.zeros(k, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(k, np.uint8))
    rs16.decode_device(k, k, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, k, engine=eng, check=True)
    assert np.array_equal(d_o.download(shape=(k, sb)), orig)
    assert np.array_equal(d_r.download(shape=(k, sb)), rec)  # the recovery stays


def _single_bit_rows(k, sb):
    """Row r holds the element 1 << (r % 16) in every position (low bytes, then high bytes per 64-byte block)."""
    orig = np.zeros((k, sb // 64, 2, 32), np.uint8)
    for bit in range(16):
        orig[bit::16, :, bit >> 3, :] = 1 << (bit & 7)
    return orig.reshape(k, sb)


@gpu
@pytest.mark.parametrize("n", [16384, 32768])
def test_single_bit_rows(n):
    # a wrong column of B (or a wrong pool entry) shows as the rows of one bit
    sb = 512
    assert _forms(n, sb, n, 0) == (1, 1)
    orig, want = _stripe(n, n, sb, _single_bit_rows(n, sb), key=("bits", n, sb))
    eng = _engine(0)
    got = _encode(eng, n, n, sb, orig, want)
    assert np.array_equal(got, want)
    # the same stripe back through the identity decode; a bit's rows are named if they differ
    d_o = DeviceArray.from_numpy(eng, np.full(n * sb, 0xA5, np.uint8))
    d_r = DeviceArray.from_numpy(eng, want)
    d_of = DeviceArray.from_numpy(eng, np.zeros(n, np.uint8))
    d_rf = DeviceArray.from_numpy(eng, np.ones(n, np.uint8))
    rs16.decode_device(n, n, sb, d_o.ptr, d_of.ptr, d_r.ptr, d_rf.ptr, 0, n, engine=eng)
    back = d_o.download(shape=(n, sb))
    bad = sorted({int(r) % 16 for r in np.nonzero((back != orig).any(axis=1))[0]})
    assert not bad, "rows of the single-bit elements 1 << %s restored wrongly" % bad


@gpu
@pytest.mark.parametrize("diag", FORMS)
@pytest.mark.parametrize("k,sb", [(10000, 512), (20000, 512), (20000, 1024)])
def test_row_limit_inside_last_tile(k, sb, diag):
    # k = m = 625 x 16 / 1250 x 16: the first pass's row limit and the last
    # pass's out_rows cut a 128-row tile between two waves -- zero-page waves in
    # the gather, masked stores in the last pass -- and the sequence is still paired
    assert k % 128 and k % 16 == 0
    assert _forms(_chunk(k), sb, k, diag) == (1, 0 if diag else 1)
    orig, want = _stripe(k, k, sb)
    assert np.array_equal(_encode(_engine(diag), k, k, sb, orig, want), want)


@gpu
def test_forms_alternate_on_one_engine():
    # Z keeps the last sequence's rows in that sequence's form; every sequence writes all it reads
    eng = rs16.Engine(0)
    n, sb = 16384, 512
    orig, want = _stripe(n, n, sb)
    for diag in (0, rs16.DIAG_NO_TOWER_ROWS, rs16.DIAG_NO_PAIRED_ROWS, 0, rs16.DIAG_WIDE_TWIDDLES, 0):
        eng.set_diagnostics(diag)
        assert np.array_equal(_encode(eng, n, n, sb, orig, want), want), diag
