"""Repair of a stripe against what a caller does without it.

In one process, per geometry (32768:32768 and 1000:1000 at 1 KiB shards,
device-resident) and per loss pattern: device time of rs16_repair_device and
of the composition it replaces, rs16_decode_device followed by
rs16_encode_device of the whole stripe -- for the recovery-only pattern the
encode alone.  The two candidates alternate burst by burst (hipEvent pairs
around bursts of back-to-back calls on the engine stream after a warm-up), so
both see the same box at the same time; the median, minimum and maximum burst
are printed.  Every pattern's repair is first checked against the originals
and the device encode of the full stripe.  One pattern is clustered (the last 1 % of the originals with the first 1 % of the
recovery), where the decode alone has kernels the repair does not take.  Then
the per-program times
(rs16_engine_set_profiling) of the repair beside those of a decode of the same
originals' losses: DEC_LAST_ALL beside DEC_LAST / DEC_TILE_LAST.

    python scripts/probe_repair.py [bursts] [calls per burst]
"""
import ctypes as C
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
import numpy as np  # noqa: E402

import rs16  # noqa: E402
from rs16._lib import hip_runtime  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402

hip = hip_runtime()
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def alternate_us(eng, fns, bursts, calls):
    """Microseconds per call of every candidate: [(median, min, max)], the
    candidates' bursts alternating."""
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    for fn in fns:
        for _ in range(calls):
            fn()
    eng.synchronize()
    out = [[] for _ in fns]
    for _ in range(bursts):
        for i, fn in enumerate(fns):
            hip.hipEventRecord(a, eng.stream)
            for _ in range(calls):
                fn()
            hip.hipEventRecord(b, eng.stream)
            hip.hipEventSynchronize(b)
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
            out[i].append(ms.value * 1e3 / calls)
    return [(statistics.median(o), min(o), max(o)) for o in out]


def patterns(k, m):
    rng = np.random.default_rng(k + m)
    pct = max(1, k // 100)
    one = (np.array([k // 3]), np.array([m // 3]))
    yield "1 % of each kind, scattered", rng.choice(k, pct, replace=False), rng.choice(m, pct, replace=False)
    yield "1 original + 1 recovery", one[0], one[1]
    yield "25 % of each kind", rng.choice(k, k // 4, replace=False), rng.choice(m, m // 4, replace=False)
    # clustered: the decode alone takes its direct middle pass and tile_last kernel here
    yield "1 % tail of the originals + 1 % head of the recovery", np.arange(k - pct, k), np.arange(pct)
    yield "recovery only, 1 %", np.array([], int), rng.choice(m, pct, replace=False)


def profile(eng, fn, n=10):
    eng.profile_reset()
    eng.set_profiling(True)
    for _ in range(n):
        fn()
    eng.synchronize()
    prof = {name: round(ms * 1e3 / n, 1) for name, (ms, c) in eng.profile().items() if c}
    eng.set_profiling(False)
    return prof


def geometry(eng, k, m, S, bursts, calls):
    print(f"== {k}:{m} x {S} B")
    orig = generate_original(k, S, 0)
    d_full_o, d_full_r = DeviceArray.from_numpy(eng, orig), DeviceArray(eng, m * S)
    rs16.encode_device(k, m, S, d_full_o.ptr, d_full_r.ptr, engine=eng)
    rec = d_full_r.download(shape=(m, S))
    enc = lambda: rs16.encode_device(k, m, S, d_full_o.ptr, d_full_r.ptr, engine=eng)  # noqa: E731
    for name, lost_o, lost_r in patterns(k, m):
        of, rf = np.ones(k, np.uint8), np.ones(m, np.uint8)
        of[lost_o] = 0
        rf[lost_r] = 0
        no, nr = int(of.sum()), int(rf.sum())
        held_o, held_r = orig.copy(), rec.copy()
        held_o[of == 0] = 0xA5
        held_r[rf == 0] = 0xA5
        d_fo, d_fr = DeviceArray.from_numpy(eng, of), DeviceArray.from_numpy(eng, rf)
        x_o, x_r = DeviceArray.from_numpy(eng, held_o), DeviceArray.from_numpy(eng, held_r)  # the repair's arrays
        y_o, y_r = DeviceArray.from_numpy(eng, held_o), DeviceArray.from_numpy(eng, held_r)  # the composition's
        rep = lambda: rs16.repair_device(k, m, S, x_o.ptr, d_fo.ptr, x_r.ptr, d_fr.ptr, no, nr, engine=eng)  # noqa: E731
        rep()
        ok = np.array_equal(x_o.download(shape=(k, S)), orig) and np.array_equal(x_r.download(shape=(m, S)), rec)
        assert ok, f"repair wrong: {name}"
        path = rs16.repair_path(k, m, no, nr)

        def dec():
            rs16.decode_device(k, m, S, y_o.ptr, d_fo.ptr, y_r.ptr, d_fr.ptr, no, nr, engine=eng)

        def dec_enc():  # today: restore the originals, then encode the whole stripe again
            dec()
            rs16.encode_device(k, m, S, y_o.ptr, y_r.ptr, engine=eng)

        base, base_name = (dec_enc, "decode + encode") if len(lost_o) else (enc, "encode alone")
        (r_med, r_min, r_max), (b_med, b_min, b_max) = alternate_us(eng, [rep, base], bursts, calls)
        print(f"{name} (lost {len(lost_o)} + {len(lost_r)}; path {path[0]}, last-pass tiles 2^{path[1]} x {path[3]}): ok")
        print(f"  repair_device        {r_med:8.2f} us  (min {r_min:.2f} max {r_max:.2f})")
        print(f"  {base_name:20s} {b_med:8.2f} us  (min {b_min:.2f} max {b_max:.2f})   "
              f"repair = {r_med / b_med:4.2f} x, {r_med - b_med:+.2f} us")
        print(f"  programs, repair: {profile(eng, rep)}")
        if len(lost_o):
            print(f"  programs, decode: {profile(eng, dec)}")


def main():
    bursts = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    eng = rs16.Engine(0)
    print(f"probe_repair: {bursts} alternating bursts of {calls} calls per candidate, hipEvent time per call, "
          "median (min max); programs: us per launch group and call")
    for k, m, S in ((32768, 32768, 1024), (1000, 1000, 1024)):
        geometry(eng, k, m, S, bursts, calls)
    eng.close()


if __name__ == "__main__":
    main()
