"""The window / batch delta update against loops of single updates.

    python scripts/probe_update_batch.py BASELINE_LIBRS16_SO [UNPACKED_LIBRS16_SO] [rounds] [bursts] [calls per burst]

The baseline is another build of the library -- the commit before
rs16_update_device_batch, built into a side directory -- never this build's
single call.  UNPACKED is this commit built with
EXTRA=-DRS16_UPDATE_BATCH_PACK_QROW=0 (no packed form of narrow windows).

The driver starts one worker process per library and round, this build's and
the other's in turn (RS16_LIB selects the library; one process at a time), and
pairs round i of one with round i of the other.  A worker measures the
hipEvent time per call of its candidates, burst by burst in alternation after
a warm-up (probe_verify.alternate_all: first the candidates both builds have,
then this build's own), and prints the median burst of each:

  whole shards, N stripes   both builds: rs16_update_device on stripe 0; N
                            such calls, one per stripe.  This build:
                            rs16_update_device_batch on the N stripes
  a window of wide shards   both builds: rs16_update_device on the whole
                            shards with deltas that are zero outside the
                            window (all the baseline can do).  This build:
                            rs16_update_device_batch on the window
  narrow windows, N stripes this build and UNPACKED: rs16_update_device_batch

Where the buffers are at most 128 MiB, the batch call's bytes are first
compared with the loop's (the padded update's) on the same inputs.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
sys.path.insert(0, str(ROOT / "scripts"))

NS = (1, 4, 16)
# (kind, k, m, shard bytes, window bytes, stripes)
MAIN = ([("whole", 1000, 1000, 1024, 1024, s) for s in (1, 4, 8, 32)] +
        [("whole", 32768, 32768, 1024, 1024, s) for s in (1, 4)] +
        [("window", 1000, 1000, 65536, 4096, 1), ("window", 8000, 8000, 65536, 4096, 1)])
PACK = [("narrow", 1000, 1000, 1024, w, 32) for w in (64, 128, 256)]
NEW_SYMBOLS = ("rs16_update_device_batch", "rs16_host_update_batch_consts")
COL = 128  # the window's column offset


def worker(which, bursts, calls):
    import ctypes as C

    import numpy as np

    from rs16 import _lib

    batch = hasattr(C.CDLL(str(_lib.LIB_PATH)), NEW_SYMBOLS[0])
    if not batch:  # a baseline library: load it without the new calls
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    import rs16
    from probe_verify import alternate_all
    from rs16.device import DeviceArray

    eng = rs16.Engine(0)
    rng = np.random.default_rng(1)
    for kind, k, m, S, W, ns in (MAIN if which == "main" else PACK):
        rec = rng.integers(0, 256, ns * m * S, dtype=np.uint8)
        for n in NS:
            plan = rs16.UpdatePlan(k, m, list(range(3, 3 + n)), engine=eng)
            win = rng.integers(0, 256, (ns, n, W), dtype=np.uint8)
            full = np.zeros((ns, n, S), np.uint8)  # the deltas as whole shards, zero outside the window
            col = 0 if W == S else COL
            full[:, :, col:col + W] = win
            d_rec, d_full, d_win = DeviceArray.from_numpy(eng, rec), DeviceArray.from_numpy(eng, full), \
                DeviceArray.from_numpy(eng, win)

            def single():
                plan.apply(S, d_full.ptr, d_rec.ptr)

            def loop():
                for i in range(ns):
                    plan.apply(S, d_full.ptr + i * n * S, d_rec.ptr + i * m * S)

            def batch_call():
                plan.apply_batch(W, ns, d_win.ptr, W, n * W, d_rec.ptr + col, S, m * S)

            out = {"kind": kind, "k": k, "m": m, "S": S, "W": W, "ns": ns, "n": n}
            if batch:
                c = (C.c_uint32 * 6)()
                assert _lib.lib().rs16_host_update_batch_consts(m, W, n, ns, c)
                out["consts"] = list(c)
            if rec.nbytes <= 1 << 27:
                # (the same calls and copies in a baseline process, so that both time in the same surroundings)
                loop()
                want = d_rec.download()
                d_rec.upload(rec)
                batch_call() if batch else loop()
                assert np.array_equal(d_rec.download(), want) and not np.array_equal(want, rec), \
                    f"batch differs from the loop: {out}"
            shared = [] if kind == "narrow" else [("single", single)] + ([("loop", loop)] if ns > 1 else [])
            t = alternate_all(eng, [fn for _, fn in shared], bursts, calls) if shared else []
            names = [name for name, _ in shared]
            if batch:
                t += alternate_all(eng, [batch_call], bursts, calls)
                names.append("batch")
            out["us"] = {name: [float(np.median(x)), float(min(x)), float(max(x))] for name, x in zip(names, t)}
            print("RESULT " + json.dumps(out), flush=True)
            plan.close()
            del d_rec, d_full, d_win
    eng.close()


def run_worker(lib, which, bursts, calls):
    env = dict(os.environ)
    if lib:
        env["RS16_LIB"] = str(lib)
    else:
        env.pop("RS16_LIB", None)
    p = subprocess.run([sys.executable, __file__, "--worker", which, str(bursts), str(calls)], env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode:
        sys.exit(f"worker failed ({lib or 'this build'}): exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    print(f"worker done: {which}, {lib or 'this build'}", file=sys.stderr, flush=True)
    return [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")]


def main():
    import numpy as np

    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    libs = [Path(a).resolve() for a in sys.argv[1:] if not a.isdigit()]
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    if not libs or not all(p.exists() for p in libs):
        sys.exit(__doc__)
    base, unpacked = libs[0], (libs[1] if len(libs) > 1 else None)
    rounds, bursts, calls = (nums + [5, 9, 20][len(nums):])[:3]
    print(f"probe_update_batch: {rounds} rounds of one process per build in turn (this build, then {base.name} of "
          f"{base.parent.name}); per process {bursts} alternating bursts of {calls} calls per candidate; hipEvent us "
          "per call: the median over the rounds of the processes' median bursts (smallest round, largest round)")
    new, old = [], []
    for _ in range(rounds):
        new.append(run_worker(None, "main", bursts, calls))
        old.append(run_worker(base, "main", bursts, calls))

    def col(runs, i, name):
        return np.array([r[i]["us"][name][0] for r in runs])

    def show(x):
        return f"{np.median(x):8.2f} ({x.min():.2f} {x.max():.2f})"

    def pairs(a, b):
        return f"faster in {int((a < b).sum())} of {len(a)} pairs"

    for i, cfg in enumerate(new[0]):
        ns, W, S = cfg["ns"], cfg["W"], cfg["S"]
        what = f"{ns} x {cfg['k']}:{cfg['m']} x {S} B" if W == S else f"{W} B window of {cfg['k']}:{cfg['m']} x {S} B"
        print(f"== {what}, n = {cfg['n']}   (Q, slabs, rows per wave, stripes per wave, waves, workgroups) = "
              f"{tuple(cfg['consts'])}")
        s_new, s_old, b_new = col(new, i, "single"), col(old, i, "single"), col(new, i, "batch")
        inside = s_old.min() <= np.median(s_new) <= s_old.max()
        label = "rs16_update_device" + ("" if W == S else ", padded")
        print(f"  {label:28s} this build {show(s_new)}   baseline {show(s_old)}   this build's median "
              f"{'inside' if inside else 'OUTSIDE'} the baseline's spread; slower in {int((s_new > s_old).sum())} of "
              f"{rounds} pairs")
        if ns > 1:
            l_new, l_old = col(new, i, "loop"), col(old, i, "loop")
            print(f"  {'loop of %d single calls' % ns:28s} this build {show(l_new)}   baseline {show(l_old)}")
            print(f"  {'rs16_update_device_batch':28s} {show(b_new)} = {np.median(b_new) / ns:.2f} per stripe, "
                  f"{np.median(l_old) / np.median(b_new):.2f} x the baseline's loop; {pairs(b_new, l_old)}")
        else:
            inside = s_old.min() <= np.median(b_new) <= s_old.max()
            print(f"  {'rs16_update_device_batch':28s} {show(b_new)}, {np.median(s_old) / np.median(b_new):.2f} x the "
                  f"baseline's {'single call' if W == S else 'padded update'}; median "
                  f"{'inside' if inside else 'OUTSIDE'} its spread; {pairs(b_new, s_old)}")
    if unpacked:
        print(f"== narrow windows: this build (packed) against {unpacked.name} of {unpacked.parent.name} (unpacked), "
              "in turn")
        pk, un = [], []
        for _ in range(rounds):
            pk.append(run_worker(None, "pack", bursts, calls))
            un.append(run_worker(unpacked, "pack", bursts, calls))
        for i, cfg in enumerate(pk[0]):
            a, b = col(pk, i, "batch"), col(un, i, "batch")
            print(f"  {cfg['ns']} x {cfg['W']} B window of {cfg['k']}:{cfg['m']} x {cfg['S']} B, n = {cfg['n']}: packed "
                  f"{tuple(cfg['consts'])} {show(a)}   unpacked {tuple(un[0][i]['consts'])} {show(b)}   packed "
                  f"{pairs(a, b)}")


if __name__ == "__main__":
    main()
