"""The multi-rank JSON line of bench.py, on CPU.

`bench.py --gpus 2 --cpu-stub` goes through the driver's launch form
(torch.distributed.run, one process per rank, gloo control plane) and the
same barrier / max-over-ranks / per-rank helpers as the GPU run, around a
numpy stand-in step.  The line must name every rank -- host, local rank,
device, its own time per step -- and the configs[4] per-rank codec times, so
that a straggler in the first 8-GPU run can be identified."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def run_stub(gpus, *more):
    env = dict(os.environ)
    for v in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", str(gpus), "--cpu-stub", "--steps", "6",
                          "--warmup", "1", *more], capture_output=True, text=True, timeout=240, env=env, cwd=str(ROOT))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout  # one JSON line, from rank 0 only
    return json.loads(lines[0])


@pytest.mark.parametrize("gpus", [1, 2])
def test_bench_line_names_every_rank(gpus):
    out = run_stub(gpus)
    assert out["stub"] is True and out["n_gpus"] == gpus
    ranks = out["ranks"]
    assert [r["rank"] for r in ranks] == list(range(gpus))
    for r in ranks:
        for key in ("hostname", "local_rank", "device", "pid", "ms_per_step", "gib_s"):
            assert key in r, key
        assert r["ms_per_step"] > 0 and r["gib_s"] > 0
    assert sorted(r["local_rank"] for r in ranks) == list(range(gpus))
    # the metric's time is the slowest rank's
    assert out["ms_per_step"] == pytest.approx(max(r["ms_per_step"] for r in ranks), rel=1e-3)
    codec = out["extra"]["configs4_rccl"]["codec_ms_per_rank"]
    assert len(codec) == gpus and all(t > 0 for t in codec)


def test_dump_outputs_files(tmp_path):
    """--dump-outputs writes float32 / float64 .npy files, the same in every
    run with the same arguments."""
    import numpy as np

    run_stub(1, "--dump-outputs", str(tmp_path / "a"))
    run_stub(1, "--dump-outputs", str(tmp_path / "b"))
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["stub.npy", "stub_rowsums.npy"]
    for name in names:
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == (np.float64 if "rowsums" in name else np.float32)
        assert np.array_equal(a, b)


def test_dump_outputs_sample(tmp_path, monkeypatch):
    """dump_outputs on an array larger than the sample: a fixed choice of whole
    rows that holds the first and the last one, the row sums of every row."""
    import numpy as np

    monkeypatch.syspath_prepend(str(ROOT))
    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE_VALUES", 64 * 10)
    a = np.random.default_rng(5).integers(0, 256, (37, 64), dtype=np.uint8)
    bench.dump_outputs(tmp_path / "x", {"big": a, "small": a[:7]})
    bench.dump_outputs(tmp_path / "y", {"big": a})
    big = np.load(tmp_path / "x" / "big.npy")
    assert big.dtype == np.float32 and big.shape[1] == 64 and 2 <= big.shape[0] <= 10
    assert np.array_equal(big, np.load(tmp_path / "y" / "big.npy"))
    assert np.array_equal(big[0], a[0]) and np.array_equal(big[-1], a[-1])
    rows = [int(np.flatnonzero((a == r).all(axis=1))[0]) for r in big]
    assert rows == sorted(set(rows))  # distinct rows, in row order
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), a[:7])
    sums = np.load(tmp_path / "x" / "big_rowsums.npy")
    assert sums.dtype == np.float64 and sums.shape == (37, 2)
    assert np.array_equal(sums[:, 0], a.sum(axis=1))
    assert np.array_equal(sums[:, 1], (a.astype(np.int64) * np.arange(1, 65)).sum(axis=1))
