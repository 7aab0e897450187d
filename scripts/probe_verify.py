"""The scrub's two paths against each other and against an encode.

In one process, per geometry (device-resident stripes), clean and with one
original corrupted (every recovery row then differs in that column block: every
lane of it stores flags): device time of rs16_verify_device on the fused path
(RS16_DIAG_FORCE_FUSED_VERIFY), on the encode + compare path
(RS16_DIAG_NO_FUSED_VERIFY), and of rs16_encode_device alone -- what the check
costs over an encode.  The three alternate burst by burst
(probe_repair.alternate_us: hipEvent pairs around bursts of back-to-back calls
on the engine stream after a warm-up); median, minimum and maximum burst are
printed, and in how many of the alternating pairs the fused path was the faster
one.  Every candidate's flags are first checked against a host comparison of
the device encode with the stored shards.  Then the per-program times
(rs16_engine_set_profiling) of the three.  Where no comparing kernel exists for
the shape (rs16_host_verify_path) the fused candidate is left out, and run
under RS16_DIAG_NO_COLUMN as well where that gives it one.

    python scripts/probe_verify.py [bursts] [calls per burst]
"""
import ctypes as C
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import numpy as np  # noqa: E402

import rs16  # noqa: E402
from probe_repair import hip, profile  # noqa: E402
from rs16.device import DeviceArray  # noqa: E402
from rs16.util import generate_original  # noqa: E402

NO, FORCE, NOCOL = rs16.DIAG_NO_FUSED_VERIFY, rs16.DIAG_FORCE_FUSED_VERIFY, rs16.DIAG_NO_COLUMN


def alternate_all(eng, fns, bursts, calls):
    """Microseconds per call of every candidate, burst by burst: [[burst 0, burst 1, ...]]."""
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
    return out


def stats(x):
    return f"{np.median(x):8.2f} us  (min {min(x):.2f} max {max(x):.2f})"


def geometry(eng, k, m, S, ns, bursts, calls, extra=0):
    tag = f"{ns} x " if ns > 1 else ""
    print(f"== {tag}{k}:{m} x {S} B" + (" under NO_COLUMN" if extra & NOCOL else ""))
    o_stride, r_stride, blocks = k * S, m * S, S // 64
    orig = np.concatenate([generate_original(k, S, i) for i in range(ns)])
    d_o, d_r, d_scratch = DeviceArray.from_numpy(eng, orig), DeviceArray(eng, ns * r_stride), DeviceArray(eng, ns * r_stride)
    d_rows, d_cols = DeviceArray(eng, ns * m), DeviceArray(eng, ns * blocks)

    def enc_into(d):
        if ns > 1:
            rs16.encode_device_batch(k, m, S, ns, d_o.ptr, o_stride, d.ptr, r_stride, engine=eng)
        else:
            rs16.encode_device(k, m, S, d_o.ptr, d.ptr, engine=eng)

    def vfy():
        if ns > 1:
            rs16.verify_device_batch(k, m, S, ns, d_o, o_stride, d_r, r_stride, d_rows, m, d_cols, blocks, engine=eng)
        else:
            rs16.verify_device(k, m, S, d_o, d_r, d_rows, d_cols, engine=eng)

    def with_diag(diag):
        def f():
            old = eng.set_diagnostics(diag | extra)
            vfy()
            eng.set_diagnostics(old)
        return f

    eng.set_diagnostics(extra)
    enc_into(d_r)  # the stored recovery: the encode of the clean originals
    eng.synchronize()
    fusable = rs16.verify_path(k, m, S, ns, diag=FORCE | extra) == 1
    for state in ("clean", "one original corrupted"):
        if state != "clean":
            bad = orig.copy()
            bad[k // 2, S // 2 + 3] ^= 0x10  # stripe 0, original k / 2
            d_o.upload(bad)
        # what a caller does today, on the host: encode into a second array, compare
        enc_into(d_scratch)
        diff = d_scratch.download(shape=(ns, m, S)) != d_r.download(shape=(ns, m, S))
        want_rows = diff.any(axis=2).astype(np.uint8)
        want_cols = diff.reshape(ns, m, blocks, 64).any(axis=(1, 3)).astype(np.uint8)
        cands = ([("fused", with_diag(FORCE))] if fusable else []) + [("encode + compare", with_diag(NO))]
        for name, fn in cands + [("default gate", with_diag(0))]:
            d_rows.upload(np.full(ns * m, 0xA5, np.uint8))
            d_cols.upload(np.full(ns * blocks, 0xA5, np.uint8))
            fn()
            ok = np.array_equal(d_rows.download(shape=(ns, m)), want_rows) and \
                np.array_equal(d_cols.download(shape=(ns, blocks)), want_cols)
            assert ok, f"verify wrong: {state}, {name}"
        cands.append(("encode alone", lambda: enc_into(d_scratch)))
        t = alternate_all(eng, [fn for _, fn in cands], bursts, calls)
        print(f"{state} (rows flagged {int(want_rows.sum())}, column blocks flagged {int(want_cols.sum())}; "
              f"default path {rs16.verify_path(k, m, S, ns, diag=extra)}): ok")
        for (name, _), x in zip(cands, t):
            print(f"  {name:18s} {stats(x)}")
        if fusable:
            f, c = np.array(t[0]), np.array(t[1])
            print(f"  fused = {np.median(f) / np.median(c):4.2f} x encode + compare, {np.median(f) - np.median(c):+.2f} us; "
                  f"faster in {int((f < c).sum())} of {len(f)} alternating pairs; "
                  f"over the encode: fused {np.median(f) - np.median(t[2]):+.2f} us, "
                  f"encode + compare {np.median(c) - np.median(t[2]):+.2f} us")
        else:
            print(f"  no comparing kernel for this shape: encode + compare over the encode "
                  f"{np.median(t[0]) - np.median(t[1]):+.2f} us")
        if state == "clean":
            for name, fn in cands:
                print(f"  programs, {name}: {profile(eng, fn)}")
    d_o.upload(orig)
    eng.set_diagnostics(0)


def main():
    bursts = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    eng = rs16.Engine(0)
    print(f"probe_verify: {bursts} alternating bursts of {calls} calls per candidate, hipEvent time per call, "
          "median (min max); programs: us per launch group and call")
    for k, m, S, ns, extra in ((32768, 32768, 1024, 1, 0), (8000, 8000, 1024, 1, 0), (60000, 3000, 1024, 1, 0),
                               (5, 3000, 1024, 1, 0), (1000, 1000, 1024, 1, 0), (1000, 1000, 1024, 1, NOCOL),
                               (1000, 1000, 1024, 4, 0), (1000, 1000, 1024, 8, 0), (1000, 1000, 1024, 32, 0)):
        geometry(eng, k, m, S, ns, bursts, calls, extra)
    eng.close()


if __name__ == "__main__":
    main()
