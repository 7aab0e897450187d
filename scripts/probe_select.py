"""Degraded read against the decode it replaces.

In one process, per geometry (32768:32768 and 1000:1000 at 1 KiB shards,
device-resident), per loss pattern (1 % of the originals scattered over every
tile, a random 50 %, every original) and per read set (one lost row, the lost
rows of one 256-row tile up to 16, every second lost row): device time of
rs16_decode_device_select and of the call it replaces, rs16_decode_device on
the same stripe and pattern.  The two alternate burst by burst
(probe_repair.alternate_us: hipEvent pairs around bursts of back-to-back calls
on the engine stream after a warm-up); median, minimum and maximum burst are
printed.  Every select is first checked: wanted rows restored, the other lost
rows untouched.  Then the per-program times (rs16_engine_set_profiling) of both
for the one-row read at scattered 1 %.

    python scripts/probe_select.py [bursts] [calls per burst]
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

import rs16  # noqa: E402
from probe_repair import alternate_us, profile  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402


def patterns(k):
    rng = np.random.default_rng(k)
    pct = max(1, k // 100)
    yield "scattered 1 %", (np.arange(pct) * (k // pct) + 7) % k
    yield "random 50 %", rng.choice(k, k // 2, replace=False)
    yield "every original", np.arange(k)


def read_sets(lost):
    lost = np.sort(lost)
    mid = lost[len(lost) // 2]
    yield "1 row", np.array([mid])
    tile = lost[lost >> 8 == mid >> 8][:16]
    yield f"{len(tile)} rows of one tile", tile
    yield "every second lost row", lost[::2]


def geometry(eng, k, m, S, bursts, calls):
    print(f"== {k}:{m} x {S} B")
    orig = generate_original(k, S, 0)
    d_full_o, d_rec = DeviceArray.from_numpy(eng, orig), DeviceArray(eng, m * S)
    rs16.encode_device(k, m, S, d_full_o.ptr, d_rec.ptr, engine=eng)
    d_fr = DeviceArray.from_numpy(eng, np.ones(m, np.uint8))
    for pname, lost in patterns(k):
        of = np.ones(k, np.uint8)
        of[lost] = 0
        no = int(of.sum())
        held = orig.copy()
        held[of == 0] = 0xA5
        d_fo = DeviceArray.from_numpy(eng, of)
        y_o = DeviceArray.from_numpy(eng, held)  # the decode's array

        def dec():
            rs16.decode_device(k, m, S, y_o.ptr, d_fo.ptr, d_rec.ptr, d_fr.ptr, no, m, engine=eng)

        for rname, rows in read_sets(lost):
            w = np.zeros(k, np.uint8)
            w[rows] = 1
            d_w = DeviceArray.from_numpy(eng, w)
            x_o = DeviceArray.from_numpy(eng, held)  # the select's array
            nw = len(rows)

            def sel():
                rs16.decode_device_select(k, m, S, x_o.ptr, d_fo.ptr, d_w.ptr, d_rec.ptr, d_fr.ptr, no, m, nw, engine=eng)

            sel()
            want = held.copy()
            want[rows] = orig[rows]
            assert np.array_equal(x_o.download(shape=(k, S)), want), f"select wrong: {pname}, {rname}"
            (s_med, s_min, s_max), (d_med, d_min, d_max) = alternate_us(eng, [sel, dec], bursts, calls)
            verdict = "below" if s_med < d_min else "NOT below"
            print(f"{pname} (lost {len(lost)}), read {rname} (wanted {nw}; path {rs16.select_path(k, m, no, m, nw)}): ok")
            print(f"  decode_device_select {s_med:8.2f} us  (min {s_min:.2f} max {s_max:.2f})")
            print(f"  decode_device        {d_med:8.2f} us  (min {d_min:.2f} max {d_max:.2f})   "
                  f"select = {s_med / d_med:4.2f} x, {s_med - d_med:+.2f} us; its median is {verdict} the decode's minimum")
            if pname == "scattered 1 %" and rname == "1 row":
                print(f"  programs, select: {profile(eng, sel)}")
                print(f"  programs, decode: {profile(eng, dec)}")


def main():
    bursts = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    eng = rs16.Engine(0)
    print(f"probe_select: {bursts} alternating bursts of {calls} calls per candidate, hipEvent time per call, "
          "median (min max); programs: us per launch group and call")
    for k, m, S in ((32768, 32768, 1024), (1000, 1000, 1024)):
        geometry(eng, k, m, S, bursts, calls)
    eng.close()


if __name__ == "__main__":
    main()
