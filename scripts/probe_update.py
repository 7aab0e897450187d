"""Delta update of recovery shards against a full re-encode.

In one process, per geometry (32768:32768 and 1000:1000 at 1 KiB shards, and
32768:32768 at 64 / 192 B for the narrow-row form): device time of
rs16_encode_device (the baseline: its code is what the parent commit has),
of rs16_update_device at n = 1, 2, 4, 8, 16, 32 changed originals, and the
host time of rs16_update_plan_new.  Device times are hipEvent pairs around
bursts of back-to-back calls on the engine stream after a warm-up; the
median, minimum and maximum burst are printed.  The update of n = 32 is first
checked against the device encode of the rewritten stripe.

    python scripts/probe_update.py [bursts] [calls per burst]
"""
import ctypes as C
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
import numpy as np  # noqa: E402

import rs16  # noqa: E402
from rs16._lib import hip_runtime  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s

hip = hip_runtime()
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]


def burst_us(eng, fn, bursts, calls):
    """Microseconds per call: (median, min, max) over `bursts` bursts."""
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    for _ in range(calls):
        fn()
    eng.synchronize()
    out = []
    for _ in range(bursts):
        hip.hipEventRecord(a, eng.stream)
        for _ in range(calls):
            fn()
        hip.hipEventRecord(b, eng.stream)
        hip.hipEventSynchronize(b)
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0
        out.append(ms.value * 1e3 / calls)
    return statistics.median(out), min(out), max(out)


def geometry(eng, k, m, S, bursts, calls):
    print(f"== {k}:{m} x {S} B")
    old = generate_original(k, S, 0)
    rng = np.random.default_rng(1)
    d_old, d_rec = DeviceArray.from_numpy(eng, old), DeviceArray(eng, m * S)
    enc = lambda: rs16.encode_device(k, m, S, d_old.ptr, d_rec.ptr, engine=eng)  # noqa: E731
    enc()
    # correctness at the timed size: update of 32 shards == device encode of the rewritten stripe
    idx = [int(i) for i in rng.choice(k, 32, replace=False)]
    new = old.copy()
    new[idx] = rng.integers(0, 256, (32, S), dtype=np.uint8)
    d_delta = DeviceArray.from_numpy(eng, old[idx] ^ new[idx])
    t0 = time.perf_counter()
    plan = rs16.UpdatePlan(k, m, idx, engine=eng)
    first_plan_ms = (time.perf_counter() - t0) * 1e3
    plan.apply(S, d_delta.ptr, d_rec.ptr)
    got = d_rec.download(shape=(m, S))
    d_new, d_rec2 = DeviceArray.from_numpy(eng, new), DeviceArray(eng, m * S)
    rs16.encode_device(k, m, S, d_new.ptr, d_rec2.ptr, engine=eng)
    assert np.array_equal(got, d_rec2.download(shape=(m, S))), "update != re-encode"
    plan.close()
    print(f"check: update(n=32) == encode(new stripe); first plan_new (cold) {first_plan_ms:.2f} ms")

    e_med, e_min, e_max = burst_us(eng, enc, bursts, calls)
    print(f"encode_device          {e_med:8.2f} us  (min {e_min:.2f} max {e_max:.2f})")
    cross = None
    for n in (1, 2, 4, 8, 16, 32):
        plan = rs16.UpdatePlan(k, m, idx[:n], engine=eng)
        upd = lambda: plan.apply(S, d_delta.ptr, d_rec.ptr)  # noqa: E731
        u_med, u_min, u_max = burst_us(eng, upd, bursts, calls)
        moved = 2 * m * S + m * n * (4 + 128) + n * S  # rows read + written, index + table lines, deltas
        line = (f"update_device n={n:<2}    {u_med:8.2f} us  (min {u_min:.2f} max {u_max:.2f})  "
                f"{u_med / e_med:5.2f} x encode  {moved / (u_med * 1e-6) / 1e12:5.2f} TB/s moved")
        if n == 1:
            line += f" = {moved / (u_med * 1e-6) / HBM_PEAK * 100:.0f} % of the 8 TB/s HBM peak"
        print(line)
        if cross is None and u_med >= e_med:
            cross = n
        plan.close()
    if cross and cross > 2:  # every n between the last two measured
        scan = []
        for n in range(cross // 2 + 1, cross + 1):
            plan = rs16.UpdatePlan(k, m, idx[:n], engine=eng)
            scan.append((n, burst_us(eng, lambda: plan.apply(S, d_delta.ptr, d_rec.ptr), bursts, calls)[0]))
            plan.close()
        print("scan: " + "  ".join(f"n={n} {u:.2f}" for n, u in scan))
        cross = next((n for n, u in scan if u >= e_med), cross)
    print("crossover: " + (f"the update stops beating the encode at n = {cross}" if cross else
                           "the update beats the encode at every n up to the cap of 32"))
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        p = rs16.UpdatePlan(k, m, idx, engine=eng)
        t.append((time.perf_counter() - t0) * 1e3)
        p.close()
    print(f"update_plan_new n=32   {statistics.median(t):8.2f} ms host time, synchronous (min {min(t):.2f} max {max(t):.2f})")


def main():
    bursts = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    eng = rs16.Engine(0)
    print(f"probe_update: {bursts} bursts of {calls} calls, hipEvent time per call, median (min max)")
    for k, m, S in ((32768, 32768, 1024), (1000, 1000, 1024), (32768, 32768, 64), (32768, 32768, 192)):
        geometry(eng, k, m, S, bursts, calls)
    eng.close()


if __name__ == "__main__":
    main()
