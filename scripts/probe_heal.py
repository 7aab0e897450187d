"""The batch locate and the heal against a loop of single locates.

The baseline is another build of the library -- the commit before the batch
forms, built into a side directory -- never this build's single calls:

    python scripts/probe_heal.py BASELINE_LIBRS16_SO [rounds] [bursts] [calls per burst]

The driver starts one worker process per library and round, this build's and
the baseline's in turn (RS16_LIB selects the library; one process at a time),
and pairs round i of one with round i of the other.  A worker measures, per
geometry (device-resident stripes, 1 KiB shards), clean and with one original
corrupted per stripe, the hipEvent time per call of its candidates, burst by
burst in alternation after a warm-up (probe_verify.alternate_all: first the
candidates both builds have, so that they run in the same surroundings in both
processes, then this build's own), and prints the median burst of each:
  both builds   rs16_locate_device on stripe 0; N rs16_locate_device calls,
                one per stripe (the loop a caller of the baseline writes)
  this build    rs16_locate_device_batch; rs16_heal_device_batch; for N = 1
                rs16_heal_device
Every candidate's answer is first checked against the construction (one
flipped bit of one original per stripe, a different shard and block in each),
and the heal with the full mask must give back the clean stripes.  In the timed
heal of the corrupted stripes the mask is RS16_HEAL_RECOVERY: the located block
names an original, so the kernel runs and counts but the stripes stay corrupted
from call to call.  Status, shard and fix of the single call go into a digest
per state, which must be equal for the two builds.

The driver prints, per geometry and state, each candidate's median over the
rounds with the smallest and largest round, the batch against the baseline's
loop pair by pair, this build's single call against the baseline's spread, and
the heal over the locate.  Then, in a process of its own, the per-program times
of this build under rs16_engine_set_profiling (which lengthens short launches).
"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "reed-solomon-16_amd"))
sys.path.insert(0, str(ROOT / "scripts"))

# (k, m, S, stripes)
SHAPES = ((1000, 1000, 1024, 1), (1000, 1000, 1024, 4), (1000, 1000, 1024, 8), (1000, 1000, 1024, 32),
          (32768, 32768, 1024, 1), (32768, 32768, 1024, 4))
NEW_SYMBOLS = ("rs16_locate_device_batch", "rs16_heal_device", "rs16_heal_device_batch",
               "rs16_host_locate_scan_shape")


def worker(mode, bursts, calls):
    import ctypes as C

    import numpy as np

    from rs16 import _lib

    # a baseline library has none of the batch forms: load it without them
    batch = hasattr(C.CDLL(str(_lib.LIB_PATH)), NEW_SYMBOLS[0])
    if not batch:
        for name in NEW_SYMBOLS:
            _lib.SIGNATURES.pop(name, None)
    import rs16
    from probe_repair import profile
    from probe_verify import alternate_all
    from rs16.device import DeviceArray
    from rs16.util import generate_original

    eng = rs16.Engine(0)
    for k, m, S, n in SHAPES:
        B = S // 64
        plan = rs16.LocatePlan(k, m, engine=eng)
        clean = np.stack([generate_original(k, S, i) for i in range(n)])
        d_o, d_r = DeviceArray.from_numpy(eng, clean), DeviceArray(eng, n * m * S)
        rs16.encode_device_batch(k, m, S, n, d_o.ptr, k * S, d_r.ptr, m * S, engine=eng)  # the stored recovery
        d_st, d_sh, d_fx = DeviceArray(eng, n * B), DeviceArray(eng, 4 * n * B), DeviceArray(eng, 64 * n * B)
        d_ct = DeviceArray(eng, 16 * n)
        eng.synchronize()

        def single():
            plan.locate(S, d_o, d_r, d_st, d_sh, d_fx)

        def loop():
            for i in range(n):
                plan.locate(S, d_o.ptr + i * k * S, d_r.ptr + i * m * S, d_st.ptr + i * B, d_sh.ptr + 4 * i * B,
                            d_fx.ptr + 64 * i * B)

        def located():
            return d_st.download(shape=(n, B)), d_sh.download(np.uint32, (n, B)), d_fx.download(shape=(n, B, 64))

        for state in ("clean", "corrupted"):
            want_st, want_sh = np.zeros((n, B), np.uint8), np.full((n, B), rs16.LOCATE_NO_SHARD, np.uint32)
            want_fx = np.zeros((n, B, 64), np.uint8)
            bad = clean.copy()
            if state == "corrupted":
                for i in range(n):
                    row, byte, val = (k // 2 + 37 * i) % k, (S // 2 + 3 + 64 * i) % S, 0x10
                    bad[i, row, byte] ^= val
                    want_st[i, byte // 64], want_sh[i, byte // 64] = rs16.LOCATE_ORIGINAL, row
                    want_fx[i, byte // 64, byte % 64] = val
                d_o.upload(bad)
            want = (want_st, want_sh, want_fx)
            mask = rs16.HEAL_RECOVERY if batch and state == "corrupted" else 3

            def batch_locate():
                plan.locate_batch(S, n, d_o, k * S, d_r, m * S, d_st, B, d_sh, B, d_fx, 64 * B)

            def batch_heal():
                plan.heal_batch(S, n, d_o, k * S, d_r, m * S, d_ct, 4, mask, d_st, B, d_sh, B)

            def single_heal():
                plan.heal(S, d_o, d_r, d_ct, mask, d_st, d_sh)

            def fill():
                for d in (d_st, d_sh, d_fx, d_ct):
                    d.upload(np.full(d.nbytes, 0xA5, np.uint8))

            cands = [("single", single)] + ([("loop", loop)] if n > 1 else [])
            if batch:
                cands += [("batch", batch_locate), ("heal_batch", batch_heal)] + \
                    ([("heal", single_heal)] if n == 1 else [])
            digest = None
            for name, fn in cands:
                fill()
                fn()
                got = located()
                rows = 1 if name in ("single", "heal") else n
                for g, w in zip(got[:2] if name.startswith("heal") else got, want):
                    assert np.array_equal(g[:rows], w[:rows]), f"{name} wrong: {k}:{m} x {n} {state}"
                if name == "single":
                    digest = hashlib.sha256(b"".join(np.ascontiguousarray(g[:1]).tobytes() for g in got)).hexdigest()
                if name.startswith("heal"):
                    counts = d_ct.download(np.uint32, (n, 4))[:rows]
                    dirty = int(state == "corrupted")
                    assert (counts == [B - dirty, dirty, 0, 0]).all(), f"{name} counts: {counts}"
            if batch and state == "corrupted":
                # the full mask once: the clean stripes come back; then the corrupted ones again
                plan.heal_batch(S, n, d_o, k * S, d_r, m * S, d_ct, 4, 3)
                assert np.array_equal(d_o.download(shape=clean.shape), clean), "heal did not restore the stripes"
                d_o.upload(bad)
            out = {"k": k, "m": m, "S": S, "n": n, "state": state, "digest": digest}
            if mode == "time":
                # the candidates both builds have alternate among themselves, the same way in
                # both processes; then this build's own
                shared = 2 if n > 1 else 1
                t = alternate_all(eng, [fn for _, fn in cands[:shared]], bursts, calls)
                if batch:
                    t += alternate_all(eng, [fn for _, fn in cands[shared:]], bursts, calls)
                out["us"] = {name: [float(np.median(x)), float(min(x)), float(max(x))] for (name, _), x in zip(cands, t)}
            else:
                out["programs"] = {name: profile(eng, fn) for name, fn in cands if name != "loop"}
            print("RESULT " + json.dumps(out), flush=True)
        d_o.upload(clean)
        plan.close()
    eng.close()


def run_worker(lib, mode, bursts, calls):
    env = dict(os.environ)
    if lib:
        env["RS16_LIB"] = str(lib)
    else:
        env.pop("RS16_LIB", None)
    p = subprocess.run([sys.executable, __file__, "--worker", mode, str(bursts), str(calls)], env=env,
                       capture_output=True, text=True, timeout=600)
    if p.returncode:
        sys.exit(f"worker failed ({lib or 'this build'}): exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
    return [json.loads(line[7:]) for line in p.stdout.splitlines() if line.startswith("RESULT ")]


def main():
    import numpy as np

    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    if len(sys.argv) < 2 or not Path(sys.argv[1]).exists():
        sys.exit(__doc__)
    base = Path(sys.argv[1]).resolve()
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    bursts = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    calls = int(sys.argv[4]) if len(sys.argv) > 4 else 20
    print(f"probe_heal: {rounds} rounds of one process per build in turn (this build, then {base.name} of "
          f"{base.parent.name}); per process {bursts} alternating bursts of {calls} calls per candidate; hipEvent us "
          "per call: the median over the rounds of the processes' median bursts (smallest round, largest round)")
    new, old = [], []
    for _ in range(rounds):
        new.append(run_worker(None, "time", bursts, calls))
        old.append(run_worker(base, "time", bursts, calls))

    def col(runs, i, name):
        return np.array([r[i]["us"][name][0] for r in runs])

    def show(x):
        return f"{np.median(x):8.2f} ({x.min():.2f} {x.max():.2f})"

    for i, cfg in enumerate(new[0]):
        n = cfg["n"]
        print(f"== {n} x {cfg['k']}:{cfg['m']} x {cfg['S']} B, {cfg['state']}")
        same = {r[i]["digest"] for r in new + old}
        print("  single call's status, shard and fix byte-equal in both builds: " + ("yes" if len(same) == 1 else "NO"))
        assert len(same) == 1
        s_new, s_old = col(new, i, "single"), col(old, i, "single")
        inside = s_old.min() <= np.median(s_new) <= s_old.max()
        print(f"  rs16_locate_device      this build {show(s_new)}   baseline {show(s_old)}   this build's median "
              f"{'inside' if inside else 'OUTSIDE'} the baseline's spread; slower in {int((s_new > s_old).sum())} of "
              f"{rounds} pairs")
        b_new, h_new = col(new, i, "batch"), col(new, i, "heal_batch")
        if n > 1:
            l_old, l_new = col(old, i, "loop"), col(new, i, "loop")
            print(f"  loop of {n:2d} single calls  this build {show(l_new)}   baseline {show(l_old)}")
            print(f"  rs16_locate_device_batch  {show(b_new)} = {np.median(b_new) / n:.2f} per stripe, "
                  f"{np.median(l_old) / np.median(b_new):.2f} x faster than the baseline's loop; faster in "
                  f"{int((b_new < l_old).sum())} of {rounds} pairs")
        else:
            print(f"  rs16_locate_device_batch  {show(b_new)} for one stripe")
            h1 = col(new, i, "heal")
            print(f"  rs16_heal_device          {show(h1)}, {np.median(h1) - np.median(s_new):+.2f} over the locate")
        print(f"  rs16_heal_device_batch    {show(h_new)}, {np.median(h_new) - np.median(b_new):+.2f} over the batch "
              "locate")
    print("== per-program times of this build, us per launch group and call (a process of its own)")
    for cfg in run_worker(None, "profile", bursts, calls):
        print(f"  {cfg['n']} x {cfg['k']}:{cfg['m']} x {cfg['S']} B, {cfg['state']}")
        for name, prof in cfg["programs"].items():
            print(f"    {name:10s} {prof}")


if __name__ == "__main__":
    main()
