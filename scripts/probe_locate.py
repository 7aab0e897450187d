"""The locate against the scrub of the same stripe.

In one process, per geometry (device-resident stripes, 1 KiB shards), clean and
with one original corrupted (every recovery row's syndrome is then nonzero in
one column block, which is located, scattered into the error array and
confirmed against all rows): device time of rs16_locate_device, of
rs16_verify_device on its default path and of rs16_encode_device alone.  The
three alternate burst by burst (probe_verify.alternate_all: hipEvent pairs
around bursts of back-to-back calls on the engine stream after a warm-up);
median, minimum and maximum burst are printed.  The locate's answer is first
checked against the construction.  Then the per-program times
(rs16_engine_set_profiling: hipEvent pairs around each launch group, which
lengthens short launches) of the locate and the scrub, and before all that the
host time of rs16_locate_plan_new (synchronous; wall clock around the call).

    python scripts/probe_locate.py [bursts] [calls per burst]
"""
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

import rs16  # noqa: E402
from probe_repair import profile  # noqa: E402
from probe_verify import alternate_all, stats  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402

SHAPES = ((32768, 32768, 1024), (1000, 1000, 1024))
PLANS = 5


def geometry(eng, k, m, S, bursts, calls):
    print(f"== {k}:{m} x {S} B")
    blocks = S // 64
    t = []
    for i in range(PLANS):
        t0 = time.perf_counter()
        plan = rs16.LocatePlan(k, m, engine=eng)
        t.append((time.perf_counter() - t0) * 1e3)
        if i + 1 < PLANS:
            plan.close()
    print("  rs16_locate_plan_new, host ms per call: " + " ".join(f"{x:.2f}" for x in t) +
          " (the first one includes the shape's first launches)")
    orig = generate_original(k, S, 0)
    d_o, d_r, d_scratch = DeviceArray.from_numpy(eng, orig), DeviceArray(eng, m * S), DeviceArray(eng, m * S)
    d_rows, d_cols = DeviceArray(eng, m), DeviceArray(eng, blocks)
    d_st, d_sh, d_fx = DeviceArray(eng, blocks), DeviceArray(eng, 4 * blocks), DeviceArray(eng, 64 * blocks)
    rs16.encode_device(k, m, S, d_o.ptr, d_r.ptr, engine=eng)  # the stored recovery
    eng.synchronize()

    def locate():
        plan.locate(S, d_o, d_r, d_st, d_sh, d_fx)

    def verify():
        rs16.verify_device(k, m, S, d_o, d_r, d_rows, d_cols, engine=eng)

    def encode():
        rs16.encode_device(k, m, S, d_o.ptr, d_scratch.ptr, engine=eng)

    row, byte, val = k // 2, S // 2 + 3, 0x10
    for state in ("clean", "one original corrupted"):
        want_st, want_sh = np.zeros(blocks, np.uint8), np.full(blocks, rs16.LOCATE_NO_SHARD, np.uint32)
        want_fx = np.zeros((blocks, 64), np.uint8)
        if state != "clean":
            bad = orig.copy()
            bad[row, byte] ^= val
            d_o.upload(bad)
            want_st[byte // 64], want_sh[byte // 64], want_fx[byte // 64, byte % 64] = rs16.LOCATE_ORIGINAL, row, val
        for d in (d_st, d_sh, d_fx):
            d.upload(np.full(d.nbytes, 0xA5, np.uint8))
        locate()
        ok = np.array_equal(d_st.download(), want_st) and np.array_equal(d_sh.download(np.uint32), want_sh) and \
            np.array_equal(d_fx.download(shape=(blocks, 64)), want_fx)
        assert ok, f"locate wrong: {state}"
        cands = [("locate", locate), ("verify", verify), ("encode alone", encode)]
        t = alternate_all(eng, [fn for _, fn in cands], bursts, calls)
        print(f"{state}: ok")
        for (name, _), x in zip(cands, t):
            print(f"  {name:14s} {stats(x)}")
        lo, vf, en = (np.array(x) for x in t)
        print(f"  locate = {np.median(lo) / np.median(vf):4.2f} x verify, {np.median(lo) - np.median(vf):+.2f} us; "
              f"= {np.median(lo) / np.median(en):4.2f} x encode; slower than verify in {int((lo > vf).sum())} of "
              f"{len(lo)} alternating pairs")
        for name, fn in cands[:2]:
            print(f"  programs, {name}: {profile(eng, fn)}")
    d_o.upload(orig)
    plan.close()


def main():
    bursts = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    eng = rs16.Engine(0)
    print(f"probe_locate: {bursts} alternating bursts of {calls} calls per candidate, hipEvent time per call, "
          "median (min max); programs: us per launch group and call")
    for k, m, S in SHAPES:
        geometry(eng, k, m, S, bursts, calls)
    eng.close()


if __name__ == "__main__":
    main()
