"""rs16_decode_device_select / rs16_decode_device_select_batch (include/rs16.h):
the degraded read -- a decode that restores only the lost originals named by a
read set, one byte per original.

Expected values: the originals are the test's own data, the recovery shards
handed in are the oracle's encode of them.  Every case pre-fills the lost slots
with 0xA5, puts a 64-byte guard behind each array and checks both arrays whole:
wanted lost rows exact, unwanted lost rows still 0xA5, received rows and the
whole recovery array byte-identical, guards untouched; then rs16_decode_check.
The read set lies at an odd address with 0xFF directly before and after it, its
"wanted" bytes are 1, 2, 0x80 and 0xFF in turn, and it names received
originals too (ignored).  The profile counters say which program ran.

One shape per kernel geometry (SHAPES), per shape four loss patterns, per
pattern the read sets over the sorted lost originals l: {l[0]}, {l[-1]},
l[::2], all of l (path 1, the plain decode), none -- and at 65536 work rows two
lost rows inside one 256-row tile and two at least 17 tiles apart, each under
the switches that choose the middle and the last pass's form.
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
WANTED_VALUES = np.array([1, 2, 0x80, 0xFF], np.uint8)

# what each shape reaches: the one-pass kernel at small T, high and low rate
# (3:2, 2:3); 256 work rows (100:100: the column codec, DEC_SINGLE_SEL T = 8
# under NO_COLUMN); the low rate (40:200); T = 4 last pass under NO_COLUMN
# (200:200); 2048 rows (600:300: COL_DEC_SEL at L = 11, three passes under
# NO_COLUMN); `chunk` inside a tile (3000:5, 5:3000); T = 7 (8000:8000); 65536
# rows, T = 8, mid_direct and tile_last in play (30000:30000, 32768:32768)
SHAPES = [(3, 2), (2, 3), (100, 100), (40, 200), (200, 200), (600, 300), (3000, 5), (5, 3000), (8000, 8000),
          (30000, 30000), (32768, 32768)]
ROWS = {(3, 2): 8, (2, 3): 8, (100, 100): 256, (40, 200): 512, (200, 200): 512, (600, 300): 2048, (3000, 5): 4096,
        (5, 3000): 4096, (8000, 8000): 16384, (30000, 30000): 65536, (32768, 32768): 65536}
LOW_RATE = {(2, 3), (40, 200), (5, 3000)}
PATTERNS = ("few", "exact", "all", "scattered")
PLAIN = {"DEC_LAST", "DEC_SINGLE", "COL_DEC", "DEC_TILE_LAST", "DEC_HALF_LAST", "DEC_HALF_SINGLE", "DEC_HALF_FIRST",
         "DEC_HALF_MID"}
SELECT = {"DEC_LAST_SEL", "DEC_SINGLE_SEL", "DEC_TILE_LAST_SEL", "COL_DEC_SEL"}
TILE_LAST_MAX, MID_DIRECT_MAX = 16, 4


@pytest.fixture(scope="module")
def eng():
    e = rs16.Engine(0)
    e.set_profiling(True)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def stripe(k, m, sb, seed=0):
    """(originals, oracle recovery) of one stripe, computed once, read-only."""
    original = generate_original(k, sb, 11 * k + m + seed)
    recovery = O.encode(k, m, original)
    original.setflags(write=False)
    recovery.setflags(write=False)
    return original, recovery


def has_pattern(k, m, name):
    return name != "all" or m >= k  # (every original lost needs original_count recovery shards)


@functools.lru_cache(maxsize=None)
def pattern(k, m, name):
    """(originals received, recovery received) as read-only bool arrays; at
    least original_count shards remain (asserted: no case skips)."""
    ok_o, ok_r = np.ones(k, bool), np.ones(m, bool)
    rng = np.random.default_rng(1000 * k + m)
    if name == "few":          # a few originals lost, all recovery received
        ok_o[sorted({0, min(3, k - 1), k // 2, k - 1})[:min(m, 4)]] = False
    elif name == "exact":      # exactly original_count received, losses of both kinds
        x = min(k, max(1, m // 2))
        ok_o[rng.choice(k, x, replace=False)] = False
        ok_r[rng.choice(m, m - x, replace=False)] = False
        assert not ok_o.all() and not ok_r.all() and ok_o.sum() + ok_r.sum() == k
    elif name == "all":        # every original lost: the half / identity trap
        ok_o[:] = False
    elif name == "scattered":  # every 97th original from 5 (from the last one where there are fewer than 6)
        ok_o[list(range(min(5, k - 1), k, 97))[:m]] = False
    else:
        raise ValueError(name)
    assert ok_o.sum() + ok_r.sum() >= k and not ok_o.all(), (k, m, name)
    ok_o.setflags(write=False)
    ok_r.setflags(write=False)
    return ok_o, ok_r


def read_set(k, m, name, rs):
    """The wanted lost originals (sorted indices) of read set `rs`."""
    lost = np.flatnonzero(~pattern(k, m, name)[0])
    if rs == "first":
        return lost[:1]
    if rs == "last":
        return lost[-1:]
    if rs == "alt":
        return lost[::2]
    if rs == "all":
        return lost
    if rs == "none":
        return lost[:0]
    if rs == "tile2":  # two lost rows inside one 256-row tile (the originals' segment starts on a tile)
        i = int(np.flatnonzero(lost[1:] >> 8 == lost[:-1] >> 8)[0])
        return lost[i:i + 2]
    if rs == "far2":   # two lost rows at least 17 tiles apart: beyond TILE_LAST_MAX, more than 4 middle-pass tile rows
        j = int(np.flatnonzero((lost >> 8) - (lost[0] >> 8) >= 17)[0])
        return lost[[0, j]]
    raise ValueError(rs)


class Case:
    """One stripe on the device with a loss pattern and a read set."""

    def __init__(self, eng, k, m, sb, name, wanted_rows, seed=0, off=1, values=WANTED_VALUES):
        self.k, self.m, self.sb, self.seed = k, m, sb, seed
        self.ok_o, self.ok_r = pattern(k, m, name)
        original, recovery = stripe(k, m, sb, seed)
        host_o = np.full(k * sb + GUARD, 0x5A, np.uint8)
        host_r = np.full(m * sb + GUARD, 0x5A, np.uint8)
        ho, hr = host_o[:k * sb].reshape(k, sb), host_r[:m * sb].reshape(m, sb)
        ho[:], hr[:] = original, recovery
        ho[~self.ok_o] = 0xA5
        hr[~self.ok_r] = 0xA5
        self.host_o, self.host_r = host_o, host_r
        self.want_rows = np.asarray(wanted_rows, np.int64)
        assert not self.ok_o[self.want_rows].any()
        # the read set: the wanted lost originals, and every third received original (ignored)
        w = np.zeros(k, np.uint8)
        w[self.want_rows] = 1
        w[np.flatnonzero(self.ok_o)[1::3]] = 1
        w = np.where(w != 0, values[np.arange(k) % len(values)], 0).astype(np.uint8)
        buf = np.full(off + k + 1, 0xFF, np.uint8)
        buf[off:off + k] = w
        self.d_wbuf = DeviceArray.from_numpy(eng, buf)
        self.wanted_ptr = self.d_wbuf.ptr + off
        self.d_o, self.d_r = DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, host_r)
        self.d_fo = DeviceArray.from_numpy(eng, self.ok_o.astype(np.uint8))
        self.d_fr = DeviceArray.from_numpy(eng, self.ok_r.astype(np.uint8))
        self.no, self.nr, self.nw = int(self.ok_o.sum()), int(self.ok_r.sum()), len(self.want_rows)
        self.path = rs16.select_path(k, m, self.no, self.nr, self.nw)

    def run(self, eng, check=True):
        eng.profile_reset()
        rs16.decode_device_select(self.k, self.m, self.sb, self.d_o.ptr, self.d_fo.ptr, self.wanted_ptr, self.d_r.ptr,
                                  self.d_fr.ptr, self.no, self.nr, self.nw, engine=eng, check=check)
        return {n: c for n, (_, c) in eng.profile().items() if c}

    def expected_originals(self):
        want = self.host_o.copy()
        rows = want[:self.k * self.sb].reshape(self.k, self.sb)
        rows[self.want_rows] = stripe(self.k, self.m, self.sb, self.seed)[0][self.want_rows]
        return want

    def check_whole(self):
        got_o, got_r = self.d_o.download(), self.d_r.download()
        assert np.array_equal(got_r, self.host_r), "recovery array or its guard written"
        assert (got_o[self.k * self.sb:] == 0x5A).all(), "guard block written"
        want = self.expected_originals()
        bad = np.flatnonzero((got_o[:self.k * self.sb].reshape(self.k, self.sb) !=
                              want[:self.k * self.sb].reshape(self.k, self.sb)).any(axis=1))
        # (which kind of row went wrong: wanted and not exact, unwanted or received and written)
        assert bad.size == 0, (bad[:8], np.isin(bad[:8], self.want_rows), self.ok_o[bad[:8]])


def check_programs(k, m, diag, case, launches):
    """The profile counters of one call against the path and the geometry."""
    rows = ROWS[(k, m)]
    if case.path == 0:
        assert launches == {}, launches
        return
    if case.path == 1:
        assert not (SELECT & launches.keys()) and launches, launches
        return
    assert not (PLAIN & launches.keys()), launches
    if 64 <= rows <= 2048 and not diag & rs16.DIAG_NO_COLUMN:
        assert launches == {"COL_DEC_SEL": 1}, launches
    elif rows <= 256:
        assert launches == {"EVAL_POLY": 1, "DEC_SINGLE_SEL": 1}, launches
    else:
        lo = (rows.bit_length() - 1) // 2
        want = {"EVAL_POLY": 1, "DEC_FIRST": 1, "DEC_MID": 1}
        if not diag & rs16.DIAG_NO_MID_DIRECT and case.nw <= MID_DIRECT_MAX << lo:
            want["DEC_MID_DIRECT"] = 1
        tl = lo == 8 and not diag & rs16.DIAG_NO_TILE_LAST and (case.nw <= 2048 or diag & rs16.DIAG_TILE_LAST)
        if tl:
            want["DEC_TILE_LAST_SEL"] = 1
        if not (tl and diag & rs16.DIAG_TILE_LAST):
            want["DEC_LAST_SEL"] = 1
        assert launches == want, (launches, want)


def run_case(eng, k, m, sb, name, rs, diag=0):
    case = Case(eng, k, m, sb, name, read_set(k, m, name, rs))
    old = eng.set_diagnostics(diag)
    try:
        launches = case.run(eng)
    finally:
        eng.set_diagnostics(old)
    case.check_whole()
    check_programs(k, m, diag, case, launches)
    return case


def test_shapes_are_what_they_stand_for():
    for k, m in SHAPES:
        high = bool(rs16.use_high_rate(k, m))
        assert high == ((k, m) not in LOW_RATE), (k, m)
        assert lib().rs16_decoder_work_count(1 if high else 0, k, m) == ROWS[(k, m)], (k, m)
    # every original lost, every recovery shard received at 32768:32768: the plain call's identity decode
    assert pattern(32768, 32768, "all")[1].all() and has_pattern(30000, 30000, "all")
    for k, m in ((30000, 30000), (32768, 32768)):
        for name in PATTERNS:
            a, b = read_set(k, m, name, "tile2"), read_set(k, m, name, "far2")
            assert len(a) == 2 and a[0] >> 8 == a[1] >> 8 and len(b) == 2 and (b[1] >> 8) - (b[0] >> 8) >= 17


def _cases():
    for k, m in SHAPES:
        for name in PATTERNS:
            if not has_pattern(k, m, name):
                continue
            for rs in ("first", "last", "alt", "all", "none"):
                yield pytest.param(k, m, name, rs, id=f"{k}:{m}-{name}-{rs}")


@pytest.mark.parametrize("k,m,name,rs", list(_cases()))
def test_select(eng, k, m, name, rs):
    case = run_case(eng, k, m, 64, name, rs)
    lost = k - case.no
    assert case.path == (0 if rs == "none" else (1 if case.nw == lost else 2))
    if rs == "all":
        # the read set covers every lost original: the plain decode, the same bytes
        x = Case(eng, k, m, 64, name, read_set(k, m, name, rs))
        rs16.decode_device(k, m, 64, x.d_o.ptr, x.d_fo.ptr, x.d_r.ptr, x.d_fr.ptr, x.no, x.nr, engine=eng)
        assert np.array_equal(x.d_o.download(), case.d_o.download())
        assert np.array_equal(x.d_r.download(), case.d_r.download())


def _no_column_cases():
    for k, m in ((100, 100), (40, 200), (200, 200), (600, 300)):
        for name in PATTERNS:
            if has_pattern(k, m, name):
                for rs in ("first", "last", "alt"):
                    yield pytest.param(k, m, name, rs, id=f"{k}:{m}-{name}-{rs}")


@pytest.mark.parametrize("k,m,name,rs", list(_no_column_cases()))
def test_select_pass_codec_below_2048_rows(eng, k, m, name, rs):
    """The stripes the column codec takes by default, through the passes:
    DEC_SINGLE_SEL at T = 8, DEC_LAST_SEL at T = 4 and T = 5."""
    case = run_case(eng, k, m, 64, name, rs, diag=rs16.DIAG_NO_COLUMN)
    assert case.path == (2 if case.nw < k - case.no else 1)


DIAGS_65536 = [("default", 0), ("no_mid_direct", rs16.DIAG_NO_MID_DIRECT), ("tile_last", rs16.DIAG_TILE_LAST),
               ("no_tile_last", rs16.DIAG_NO_TILE_LAST), ("fd_lds", rs16.DIAG_FD_LDS),
               ("voff64", rs16.DIAG_FORCE_VOFF64)]


def _cases_65536():
    for k, m in ((30000, 30000), (32768, 32768)):
        for name in PATTERNS:
            for rs in ("tile2", "far2"):
                for dname, diag in DIAGS_65536:
                    yield pytest.param(k, m, name, rs, diag, id=f"{k}:{m}-{name}-{rs}-{dname}")


@pytest.mark.parametrize("k,m,name,rs,diag", list(_cases_65536()))
def test_select_65536_rows(eng, k, m, name, rs, diag):
    """Each last-pass form and each middle form on both sides of its switch,
    with a read set narrower than the losses."""
    case = run_case(eng, k, m, 64, name, rs, diag=diag)
    assert case.path == 2 and case.nw == 2


@pytest.mark.parametrize("k,m,sb", [(100, 100, 192), (100, 100, 1024), (8000, 8000, 192), (8000, 8000, 1024)])
@pytest.mark.parametrize("name,rs", [("exact", "alt"), ("few", "first")])
def test_widths(eng, k, m, sb, name, rs):
    """Partial and whole slabs."""
    assert run_case(eng, k, m, sb, name, rs).path == 2


@pytest.mark.parametrize("values", [(1,), (2,), (0x80,), (0xFF,), (0x80, 1, 0xFF, 2)])
@pytest.mark.parametrize("k,m,diag", [(100, 100, 0), (200, 200, rs16.DIAG_NO_COLUMN), (3000, 5, 0),
                                      (32768, 32768, 0)])
def test_wanted_bytes(eng, k, m, diag, values):
    """Any nonzero byte means wanted, in every reader of the read set."""
    case = Case(eng, k, m, 64, "exact", read_set(k, m, "exact", "alt"), values=np.array(values, np.uint8))
    old = eng.set_diagnostics(diag)
    try:
        launches = case.run(eng)
    finally:
        eng.set_diagnostics(old)
    case.check_whole()
    check_programs(k, m, diag, case, launches)


@pytest.mark.parametrize("off", [64, 2, 3])
@pytest.mark.parametrize("k,m,name", [(100, 100, "few"), (3000, 5, "few"), (32768, 32768, "few"),
                                      (32768, 32768, "exact")])
def test_read_set_alignments(eng, k, m, name, off):
    """The read set 64-byte aligned and at every offset within a dword (the
    other cases: offset 1); 32768:32768 takes the one-kernel eval form, which
    fetches the read set as aligned dwords."""
    case = Case(eng, k, m, 64, name, read_set(k, m, name, "alt"), off=off)
    assert case.path == 2 and case.wanted_ptr % 64 == off % 64
    case.run(eng)
    case.check_whole()


@pytest.mark.parametrize("k,m,diag", [(100, 100, 0), (600, 300, rs16.DIAG_NO_COLUMN), (8000, 8000, 0)])
@pytest.mark.parametrize("name,rs", [("exact", "alt"), ("few", "last")])
def test_batch(eng, k, m, diag, name, rs):
    sb, n, gap = 64, 3, 128
    so, sr = k * sb + gap, m * sb + gap
    ok_o, ok_r = pattern(k, m, name)
    rows = read_set(k, m, name, rs)
    host_o = np.full(n * so + GUARD, 0x5A, np.uint8)
    host_r = np.full(n * sr + GUARD, 0x5A, np.uint8)
    old = eng.set_diagnostics(diag)
    try:
        singles = []
        for i in range(n):
            c = Case(eng, k, m, sb, name, rows, seed=i)
            host_o[i * so:i * so + k * sb] = c.host_o[:k * sb]
            host_r[i * sr:i * sr + m * sb] = c.host_r[:m * sb]
            c.run(eng)  # the single call on this stripe
            c.check_whole()
            singles.append(c.d_o.download()[:k * sb])
        c0 = Case(eng, k, m, sb, name, rows)  # (its flags and read set)
        d_o, d_r = DeviceArray.from_numpy(eng, host_o), DeviceArray.from_numpy(eng, host_r)
        eng.profile_reset()
        rs16.decode_device_select_batch(k, m, sb, n, d_o.ptr, so, c0.d_fo.ptr, c0.wanted_ptr, d_r.ptr, sr,
                                        c0.d_fr.ptr, c0.no, c0.nr, c0.nw, engine=eng, check=True)
        launches = {p: c for p, (_, c) in eng.profile().items() if c}
    finally:
        eng.set_diagnostics(old)
    assert c0.path == 2
    check_programs(k, m, diag, c0, launches)
    got_o, got_r = d_o.download(), d_r.download()
    assert np.array_equal(got_r, host_r)
    for i in range(n):
        assert np.array_equal(got_o[i * so:i * so + k * sb], singles[i]), i
        assert (got_o[i * so + k * sb:(i + 1) * so] == 0x5A).all(), i  # gap bytes untouched
    assert (got_o[n * so:] == 0x5A).all()


def test_sequence_on_one_engine():
    """select -> plain decode -> another read set -> decode_prepare + select:
    the preparation is discarded and every result is right."""
    eng = rs16.Engine(0)
    try:
        k = m = 4096
        sb = 64
        a = Case(eng, k, m, sb, "exact", read_set(k, m, "exact", "first"))
        a.run(eng)
        a.check_whole()
        b = Case(eng, k, m, sb, "all", read_set(k, m, "all", "all"))
        rs16.decode_device(k, m, sb, b.d_o.ptr, b.d_fo.ptr, b.d_r.ptr, b.d_fr.ptr, b.no, b.nr, engine=eng, check=True)
        b.check_whole()  # (the identity decode)
        c = Case(eng, k, m, sb, "all", read_set(k, m, "all", "alt"))
        c.run(eng)
        c.check_whole()
        d = Case(eng, k, m, sb, "scattered", read_set(k, m, "scattered", "last"))
        p = Case(eng, k, m, sb, "exact", read_set(k, m, "exact", "alt"))
        rs16.decode_prepare(k, m, sb, p.d_fo.ptr, p.d_fr.ptr, p.no, p.nr, engine=eng)  # another pattern's locator
        d.run(eng)
        d.check_whole()
        with pytest.raises(rs16.Error) as e:
            rs16.decode_device_prepared(k, m, sb, p.d_o.ptr, p.d_r.ptr, engine=eng)
        assert e.value.kind == "InvalidArgument"
        # and a plain decode of a column-codec size, then a select at the same size
        for kk in (1000, 4096):
            y = Case(eng, kk, kk, sb, "few", read_set(kk, kk, "few", "all"))
            rs16.decode_device(kk, kk, sb, y.d_o.ptr, y.d_fo.ptr, y.d_r.ptr, y.d_fr.ptr, y.no, y.nr, engine=eng,
                               check=True)
            y.check_whole()
            z = Case(eng, kk, kk, sb, "few", read_set(kk, kk, "few", "last"))
            z.run(eng)
            z.check_whole()
    finally:
        eng.close()


@pytest.mark.parametrize("k,m,name,rs,claimed", [
    (32768, 32768, "exact", "far2", 5000),    # two rows claimed as 5000: neither small kernel is launched
    (32768, 32768, "exact", "tile2", 5000),   # ... although one tile would do
    (32768, 32768, "scattered", "alt", 1),    # 169 rows over every tile claimed as one: both small kernels launched, both return
    (8000, 8000, "scattered", "alt", 1),
    (600, 300, "scattered", "alt", 1),        # the column codec has no host gate
])
def test_wrong_wanted_count_costs_time_only(eng, k, m, name, rs, claimed):
    """A wanted_count between 1 and the lost count that does not match the read
    set only steers the host's gates (include/rs16.h): the device decides by the
    interval it computes itself, and the rows restored are the arrays'."""
    case = Case(eng, k, m, 64, name, read_set(k, m, name, rs))
    assert case.nw != claimed and 0 < claimed < k - case.no
    true_nw, case.nw = case.nw, claimed
    assert rs16.select_path(k, m, case.no, case.nr, claimed) == 2
    launches = case.run(eng)
    case.check_whole()
    check_programs(k, m, 0, case, launches)  # (the gates follow the claimed count)
    assert true_nw == len(case.want_rows)


def test_slices_do_not_apply(eng):
    k, m = 8000, 8000
    case = Case(eng, k, m, 256, "scattered", read_set(k, m, "scattered", "alt"))
    eng.set_slices(4)
    try:
        launches = case.run(eng)
    finally:
        eng.set_slices(1)
    case.check_whole()
    check_programs(k, m, 0, case, launches)  # one launch of each program: one slice


def test_decode_check_reads_the_flags(eng):
    k, m, sb = 200, 200, 64
    case = Case(eng, k, m, sb, "few", read_set(k, m, "few", "first"))
    err = RS16Error()
    # a recovery count one too low is still a valid decode; the flags say otherwise
    rs16.decode_device_select(k, m, sb, case.d_o.ptr, case.d_fo.ptr, case.wanted_ptr, case.d_r.ptr, case.d_fr.ptr,
                              case.no, case.nr - 1, case.nw, engine=eng)
    rc = lib().rs16_decode_check(eng.h, None, C.byref(err))
    assert rs16.Error._from_c(err).kind == "InvalidArgument" and rc == err.code
    assert (err.v0, err.v1) == (case.no, case.nr)
    case.check_whole()


def test_errors_and_their_order(eng):
    k, m, sb = 4, 4, 64
    d_o, d_r = DeviceArray(eng, 2 * k * sb + 64), DeviceArray(eng, 2 * m * sb + 64)
    f = DeviceArray.from_numpy(eng, np.ones(8, np.uint8))
    before_o, before_r = d_o.download(), d_r.download()

    def single(**kw):
        a = dict(k=k, m=m, sb=sb, o=d_o.ptr, fo=f.ptr, w=f.ptr, r=d_r.ptr, fr=f.ptr, no=k - 2, nr=m - 1, nw=1)
        a.update(kw)
        return lambda: rs16.decode_device_select(a["k"], a["m"], a["sb"], a["o"], a["fo"], a["w"], a["r"], a["fr"],
                                                 a["no"], a["nr"], a["nw"], engine=eng)

    def batch(**kw):
        a = dict(k=k, m=m, sb=sb, n=2, o=d_o.ptr, so=k * sb, fo=f.ptr, w=f.ptr, r=d_r.ptr, sr=m * sb, fr=f.ptr,
                 no=k - 2, nr=m - 1, nw=1)
        a.update(kw)
        return lambda: rs16.decode_device_select_batch(a["k"], a["m"], a["sb"], a["n"], a["o"], a["so"], a["fo"],
                                                       a["w"], a["r"], a["sr"], a["fr"], a["no"], a["nr"], a["nw"],
                                                       engine=eng)

    def kind(call):
        with pytest.raises(rs16.Error) as e:
            call()
        return e.value

    eng.profile_reset()
    for form in (single, batch):
        # 1. rs16_validate's errors first, whatever else is wrong
        assert kind(form(k=0, o=0)) == rs16.Error("UnsupportedShardCount", original_count=0, recovery_count=m)
        assert kind(form(k=40000, m=40000, no=0, nr=0, w=0)).kind == "UnsupportedShardCount"
        assert kind(form(sb=100, o=d_o.ptr + 32, no=0, nr=0)) == rs16.Error("InvalidShardSize", shard_bytes=100)
        assert kind(form(sb=0, w=0)).kind == "InvalidShardSize"
        # 2. null / misaligned arrays, before the counts are looked at
        for bad in (dict(o=0), dict(r=0), dict(fo=0), dict(fr=0), dict(w=0), dict(o=d_o.ptr + 32),
                    dict(r=d_r.ptr + 16)):
            assert kind(form(no=0, nr=0, nw=9, **bad)).kind == "InvalidArgument", bad
        # 3. counts above their shard counts, wanted above the lost originals -- before "too few"
        assert kind(form(no=k + 1)).kind == "InvalidArgument"
        assert kind(form(nr=m + 1)).kind == "InvalidArgument"
        assert kind(form(nw=3)).kind == "InvalidArgument"
        assert kind(form(no=1, nr=2, nw=4)).kind == "InvalidArgument"
        # 4. too few received
        assert kind(form(no=1, nr=2, nw=3)) == rs16.Error("NotEnoughShards", original_count=k,
                                                          original_received_count=1, recovery_received_count=2)
        # 5. everything received, or nothing wanted: OK, nothing launched
        form(no=k, nr=0, nw=0)()
        form(nw=0)()
    # 2. (batch) bad strides, before the counts
    for bad in (dict(so=k * sb - 64), dict(sr=m * sb - 64), dict(so=k * sb + 32), dict(sr=m * sb + 32)):
        assert kind(batch(no=0, nr=0, **bad)).kind == "InvalidArgument", bad
    batch(n=0)()  # no stripes: nothing to do once the arguments are valid
    assert {n: c for n, (_, c) in eng.profile().items() if c} == {}  # all of it before any launch
    assert np.array_equal(d_o.download(), before_o) and np.array_equal(d_r.download(), before_r)
