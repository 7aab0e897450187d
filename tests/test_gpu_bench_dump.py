"""A plain `bench.py` run and its --dump-outputs files, on the GPU: the
timed steps' last outputs must be the oracle's recovery shards and the
restored originals, and the line must hold the metric's fields only."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import oracle_bind as O
from rs16.util import generate_original

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu


# 1000:1000 loses every original (half-transform decode); 300:200 keeps the
# last 100 originals in place (general decode)
@pytest.mark.parametrize("k,m", [(1000, 1000), (300, 200)])
def test_plain_bench_dump_matches_oracle(tmp_path, k, m):
    S = 1024
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--original", str(k), "--recovery", str(m), "--shard-bytes", str(S),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u16"
    assert out["full"] is False
    for key in ("extra", "cpu_baseline", "roofline", "kernels_us"):
        assert key not in out, key
    original = generate_original(k, S, 0)
    recovery = O.encode(k, m, original)
    for name, want in (("recovery", recovery), ("restored", original)):
        got = np.load(tmp_path / f"{name}.npy")
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got, want.astype(np.float32)), name
        sums = np.load(tmp_path / f"{name}_rowsums.npy")
        assert sums.dtype == np.float64
        assert np.array_equal(sums[:, 0], want.sum(axis=1))
