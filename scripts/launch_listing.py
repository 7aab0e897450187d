#!/usr/bin/env python3
"""Which programs a fixed list of calls launches, and what they compute.

One line per call: the launch counts per program name (Engine.profile()) and a
SHA-1 prefix of everything the call wrote, on seeded inputs.  Run once per
library (RS16_LIB selects it) on the same GPU; two libraries that enqueue the
same work print byte-identical listings (profiles/r21_engine_plan_launches.txt).
The calls reach every EncodeForm at both rates and every kind of decode plan;
shards of 64 .. 1024 bytes, so the whole listing takes seconds.

  RS16_LIB=<librs16.so> python scripts/launch_listing.py > listing.txt
"""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))

import rs16  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402

eng = rs16.Engine(0)
eng.set_profiling(True)


def sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:12]


def call(title, fn, results, want=None):
    """fn() enqueues the call; results() downloads what it wrote, the restored
    originals first where want is given (they must equal it)."""
    eng.synchronize()
    eng.profile_reset()
    fn()
    eng.synchronize()
    prof = " ".join("%s=%d" % (name, n) for name, (_, n) in sorted(eng.profile().items()))
    out = results()
    ok = "" if want is None else (" = the originals" if np.array_equal(out[0], want) else " WRONG")
    print("%s: [%s] results %s%s" % (title, prof, sha(*out), ok), flush=True)


def diag(flags):
    return eng.set_diagnostics(flags)


def rate(k, m):
    return "high" if rs16.use_high_rate(k, m) else "low"


def masks(k, m, pattern, seed):
    """(originals received, recovery received) as bool arrays."""
    rng = np.random.default_rng(seed)
    om, rm = np.ones(k, bool), np.zeros(m, bool)
    lost = min(k, m)
    if pattern == "all":  # every original lost, every recovery shard received
        om[:] = False
        rm[:] = True
    elif pattern == "1pct":
        n = max(1, lost // 100)
        om[k - n:] = False
        rm[:n] = True
    else:  # scatter
        n = int(rng.integers(1, lost + 1))
        om[rng.choice(k, n, replace=False)] = False
        rm[rng.choice(m, min(m, n + 2), replace=False)] = True
    return om, rm


class Stripes:
    """n stripes of k:m x sb on the device, encoded by the library under test."""

    def __init__(self, k, m, sb, n=1, seed=0):
        self.k, self.m, self.sb, self.n = k, m, sb, n
        self.original = np.stack([generate_original(k, sb, seed + i) for i in range(n)])
        self.d_o = DeviceArray.from_numpy(eng, self.original)
        self.d_r = DeviceArray(eng, n * m * sb)
        self.os, self.rs = k * sb, m * sb

    def shape(self):
        return "%s%d:%d x %d (%s)" % ("%d x " % self.n if self.n > 1 else "", self.k, self.m, self.sb,
                                     rate(self.k, self.m))

    def encode(self):
        if self.n == 1:
            rs16.encode_device(self.k, self.m, self.sb, self.d_o.ptr, self.d_r.ptr, engine=eng)
        else:
            rs16.encode_device_batch(self.k, self.m, self.sb, self.n, self.d_o.ptr, self.os, self.d_r.ptr, self.rs,
                                     engine=eng)

    def recovery(self):
        return self.d_r.download(shape=(self.n, self.m, self.sb))

    def holes(self, om):
        """Upload the originals with the lost rows overwritten; om: (k) or (n, k) bool."""
        held = self.original.copy()
        held[~np.broadcast_to(om, (self.n, self.k))] = 0xA5
        self.d_o.upload(held)

    def restored(self):
        return [self.d_o.download(shape=(self.n, self.k, self.sb))]


def encode_case(k, m, sb, n=1, note=""):
    st = Stripes(k, m, sb, n)
    call("%s encode%s" % (st.shape(), note), st.encode, lambda: [st.recovery()])
    return st


def flags(om, rm):
    return DeviceArray.from_numpy(eng, om.astype(np.uint8)), DeviceArray.from_numpy(eng, rm.astype(np.uint8))


def decode_case(k, m, sb, pattern, note="", how="decode_device", n=1):
    st = Stripes(k, m, sb, n, seed=k % 251)
    st.encode()
    om, rm = masks(k, m, pattern, k + m)
    no, nr = int(om.sum()), int(rm.sum())
    d_fo, d_fr = flags(om, rm)
    st.holes(om)
    keep = [d_fo, d_fr]
    if how == "decode_device":
        fn = lambda: rs16.decode_device(k, m, sb, st.d_o.ptr, d_fo.ptr, st.d_r.ptr, d_fr.ptr, no, nr, engine=eng)
    elif how == "decode_device_batch":
        fn = lambda: rs16.decode_device_batch(k, m, sb, n, st.d_o.ptr, st.os, d_fo.ptr, st.d_r.ptr, st.rs, d_fr.ptr,
                                              no, nr, engine=eng)
    elif how == "decode_device_select":
        want = np.zeros(k, np.uint8)
        want[np.flatnonzero(~om)[::2]] = 1  # every second lost original
        d_w = DeviceArray.from_numpy(eng, want)
        keep.append(d_w)
        fn = lambda: rs16.decode_device_select(k, m, sb, st.d_o.ptr, d_fo.ptr, d_w.ptr, st.d_r.ptr, d_fr.ptr, no, nr,
                                               int(want.sum()), engine=eng)
    elif how == "prepare + encode + prepared":
        def fn():
            rs16.decode_prepare(k, m, sb, d_fo.ptr, d_fr.ptr, no, nr, engine=eng)
            st2.encode()  # (another stripe's encode between the two halves)
            rs16.decode_device_prepared(k, m, sb, st.d_o.ptr, st.d_r.ptr, engine=eng)
        st2 = Stripes(k, m, sb, 1, seed=7)
    elif how == "repair_device":
        rec = st.recovery()
        rec[0][~rm] = 0x5A
        st.d_r.upload(rec)
        fn = lambda: rs16.repair_device(k, m, sb, st.d_o.ptr, d_fo.ptr, st.d_r.ptr, d_fr.ptr, no, nr, engine=eng)
    else:
        raise ValueError(how)
    results = (lambda: st.restored() + [st.recovery()]) if how == "repair_device" else st.restored
    # (the selective decode leaves the lost originals outside the read set as they were)
    call("%s %s, %s%s" % (st.shape(), how, pattern, note), fn, results,
         None if how == "decode_device_select" else st.original)
    del keep


def varied_case(k, m, sb, n):
    st = Stripes(k, m, sb, n, seed=3)
    st.encode()
    ms = [masks(k, m, "scatter", 100 + i) for i in range(n)]
    om, rm = np.stack([a for a, _ in ms]), np.stack([b for _, b in ms])
    d_fo, d_fr = flags(om, rm)
    st.holes(om)
    call("%s decode_device_batch_varied" % st.shape(),
         lambda: rs16.decode_device_batch_varied(k, m, sb, n, st.d_o.ptr, st.os, d_fo.ptr, k, st.d_r.ptr, st.rs,
                                                 d_fr.ptr, m, om.sum(1), rm.sum(1), engine=eng), st.restored,
         st.original)


def host_case(k, m, sb, n, slice_bytes=0):
    original = np.stack([generate_original(k, sb, 11 + i) for i in range(n)])
    recovery = np.zeros((n, m, sb), np.uint8)
    rs16.encode_host_batch(k, m, sb, n, original, k * sb, recovery, m * sb, engine=eng)
    ms = [masks(k, m, "scatter", 200 + i) for i in range(n)]
    om = np.stack([a for a, _ in ms]).astype(np.uint8)
    rm = np.stack([b for _, b in ms]).astype(np.uint8)
    held = original.copy()
    held[om == 0] = 0xA5
    shape = "%s%d:%d x %d (%s)" % ("%d x " % n if n > 1 else "", k, m, sb, rate(k, m))
    if n == 1:
        call("%s decode_host, slices of %d bytes" % (shape, slice_bytes),
             lambda: rs16.decode_host(k, m, sb, held[0], om[0], recovery[0], rm[0], slice_bytes, engine=eng),
             lambda: [held], original)
    else:
        call("%s decode_host_batch" % shape,
             lambda: rs16.decode_host_batch(k, m, sb, n, held, k * sb, om, k, recovery, m * sb, rm, m, engine=eng),
             lambda: [held], original)


def rate_decoder_case(k, m, sb, which):
    original = generate_original(k, sb, 5)
    dec =rs16.RateDecoder(k, m, sb, rate=which, engine=eng)
    enc = rs16.RateEncoder(k, m, sb, rate=which, engine=eng)
    for row in original:
        enc.add_original_shard(row)
    with enc.encode() as res:
        recovery = [res.recovery(i) for i in range(m)]
    for i in range(k):  # every original lost
        dec.add_recovery_shard(i, recovery[i])
    out = []

    def fn():
        with dec.decode() as res:
            out.append(np.stack([np.frombuffer(res.restored_original(i), np.uint8) for i in range(k)]))
    call("%d:%d x %d RateDecoder(%s), all originals lost" % (k, m, sb, which), fn,
         lambda: [out[0]], original)


NO_COL, FORCE_COL = rs16.DIAG_NO_COLUMN, rs16.DIAG_FORCE_COLUMN

print("# encode forms")
for k, m in [(1, 1), (2, 2), (100, 100), (1000, 1000), (3000, 3000),      # one-chunk high rate
             (100, 1000), (1000, 100),                                       # colm
             (3000, 1000), (300, 2000), (8000, 300),                         # column chunks
             (60000, 3000), (3000, 60000), (8000, 200),                      # passes
             (5, 1), (1, 5),                                                 # L == 0
             (1000, 600), (400, 300)]:                                       # the low rate's one column launch
    encode_case(k, m, 64)
encode_case(1000, 1000, 1024)
diag(NO_COL)
for k, m in [(1000, 1000), (100, 1000), (1000, 100), (3000, 1000), (300, 2000), (1000, 600), (20, 300), (300, 20)]:
    encode_case(k, m, 64, note=", DIAG_NO_COLUMN")
diag(FORCE_COL)
encode_case(8000, 1000, 64, note=", DIAG_FORCE_COLUMN")
diag(0)
encode_case(200, 200, 64, n=8)      # the one-chunk batch: narrow enough for the column codec
encode_case(1000, 1000, 1024, n=8)  # ... too wide: three passes
encode_case(100, 100, 1024, n=8)    # ... too wide: one pass
encode_case(600, 300, 64, n=3)      # other shapes: stripe by stripe
eng.set_slices(2)
encode_case(1000, 1000, 1024, note=", 2 column slices")
encode_case(3000, 3000, 128, note=", 2 column slices")
eng.set_slices(1)

print("# decode plans")
decode_case(2048, 2048, 64, "all", " (identity)")
decode_case(4096, 4096, 64, "all", " (identity)")
decode_case(1000, 1000, 64, "all", " (column, own evaluation)")
decode_case(400, 400, 64, "all", " (column, own evaluation)")
rate_decoder_case(500, 512, 64, "low")    # COL_DEC_EWORK, 512-row half
rate_decoder_case(1000, 1024, 64, "low")  # COL_DEC_EWORK, 1024-row half
rate_decoder_case(1000, 1000, 64, "high")
rate_decoder_case(3000, 3000, 64, "default")
diag(NO_COL)
decode_case(100, 100, 64, "all", ", DIAG_NO_COLUMN (one-pass half)")
decode_case(1000, 1000, 64, "all", ", DIAG_NO_COLUMN (three-pass half)")
decode_case(100, 100, 64, "scatter", ", DIAG_NO_COLUMN (one-pass general)")
decode_case(1000, 1000, 64, "scatter", ", DIAG_NO_COLUMN (three-pass general)")
diag(0)
decode_case(3000, 3000, 64, "all", " (three-pass half)")
decode_case(1000, 1000, 64, "1pct", " (column general)")
decode_case(200, 200, 64, "scatter", " (column general)")
decode_case(300, 1000, 64, "scatter", " (column general, low rate)")
decode_case(1000, 1000, 64, "scatter", how="decode_device_select")
decode_case(4096, 4096, 64, "scatter", how="decode_device_select")
decode_case(4096, 4096, 256, "scatter")
decode_case(300, 3000, 64, "scatter")
decode_case(32768, 32768, 128, "1pct", " (mid_direct, tile_last)")
diag(rs16.DIAG_NO_MID_DIRECT)
decode_case(32768, 32768, 128, "1pct", ", DIAG_NO_MID_DIRECT")
diag(rs16.DIAG_NO_TILE_LAST)
decode_case(32768, 32768, 128, "1pct", ", DIAG_NO_TILE_LAST")
diag(rs16.DIAG_NO_MID_DIRECT | rs16.DIAG_NO_TILE_LAST)
decode_case(32768, 32768, 128, "1pct", ", DIAG_NO_MID_DIRECT | DIAG_NO_TILE_LAST")
diag(0)
decode_case(1000, 1000, 64, "scatter", how="repair_device")
decode_case(3000, 3000, 64, "scatter", how="repair_device")
decode_case(300, 3000, 64, "scatter", how="repair_device")
decode_case(200, 200, 64, "scatter", how="decode_device_batch", n=3)
decode_case(1000, 1000, 1024, "all", how="decode_device_batch", n=3)
varied_case(200, 200, 64, 4)
varied_case(1000, 1000, 1024, 4)
eng.set_slices(2)
decode_case(2048, 2048, 128, "all", ", 2 column slices (identity)")
decode_case(1000, 1000, 1024, "all", ", 2 column slices")
decode_case(3000, 3000, 128, "scatter", ", 2 column slices")
decode_case(2048, 2048, 128, "all", ", 2 column slices", how="prepare + encode + prepared")
eng.set_slices(1)
decode_case(1000, 1000, 1024, "all", how="prepare + encode + prepared")
decode_case(4096, 4096, 256, "scatter", how="prepare + encode + prepared")
decode_case(2048, 2048, 64, "all", how="prepare + encode + prepared")
host_case(1000, 1000, 1024, 1, 512)
host_case(3000, 3000, 128, 1)
host_case(1000, 1000, 64, 4)
host_case(4096, 4096, 64, 3)
eng.close()
