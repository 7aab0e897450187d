"""The form of the work buffer Z is one decision per sequence (z_form_sequence,
rs16_pass_launch.hip), shown by two hooks: rs16_host_paired_rows (the form is
at least the paired one) and rs16_host_tower_rows (it is the tower one).  This
sweeps both over a grid and compares every answer with the answers recorded
from the library before the decision was gathered into one function
(tests/golden/z_form_sweep.json: the grid's axes and one '0' / '1' per point
and hook, nothing else).  No device needed.

The grid is the product of the fixture's axes in the order of `_points`:
chunk sizes below, at and above the gate's 512 rows, one that is no power of
two, and the 2^14 / 2^15-row chunks that have paired kernels; widths that are
and are not a multiple of 512 bytes, up to 2^20; the caller's stride equal to
and twice the width; row limits that do and do not cut through a wave; the
decode's segment boundary and first gather row at 0 and at the chunk; and the
diagnostic switches that bear on the decision.
"""
import itertools
import json
import pathlib

from rs16._lib import lib

FIXTURE = pathlib.Path(__file__).parent / "golden" / "z_form_sweep.json"

AXES = {
    "chunk_rows": [256, 512, 1000, 4096, 8192, 16384, 32768, 65536, 131072],
    "S": [8, 64, 512, 960, 1024, 4096, 1 << 20],
    "S_user_factor": [1, 2],
    "a_count": ["0", "1", "chunk_rows / 2", "chunk_rows - 1", "chunk_rows"],
    "seg_chunk": ["0", "chunk_rows"],
    "row_base_in": ["0", "chunk_rows"],
    # 0, RS16_DIAG_NO_PAIRED_ROWS, _NO_TOWER_ROWS, _NO_LATE_ROWS, _FORCE_VOFF64 (include/rs16.h)
    "diag": [0, 8192, 16384, 4096, 1],
}


def _rows(expr, chunk):
    return {"0": 0, "1": 1, "chunk_rows / 2": chunk // 2, "chunk_rows - 1": chunk - 1, "chunk_rows": chunk}[expr]


def _points(axes):
    for chunk, s, f, ac, sc, rb, diag in itertools.product(*(axes[k] for k in AXES)):
        yield chunk, s, s * f, _rows(ac, chunk), _rows(sc, chunk), _rows(rb, chunk), diag


def sweep(axes):
    """One '0' / '1' per grid point, for each of the two hooks."""
    L = lib()
    paired, tower = [], []
    for p in _points(axes):
        paired.append(str(L.rs16_host_paired_rows(*p)))
        tower.append(str(L.rs16_host_tower_rows(*p)))
    return "".join(paired), "".join(tower)


def test_decision_is_the_recorded_one():
    want = json.loads(FIXTURE.read_text())
    assert want["axes"] == AXES, "the fixture was recorded over another grid"
    n = len(list(_points(AXES)))
    assert n == 12600 and len(want["paired"]) == n and len(want["tower"]) == n
    # both outcomes are in the recorded grid, for each hook
    for hook in ("paired", "tower"):
        assert set(want[hook]) == {"0", "1"}, hook
    paired, tower = sweep(AXES)
    bad = [(p, hook) for i, p in enumerate(_points(AXES))
           for hook, got in (("paired", paired), ("tower", tower)) if got[i] != want[hook][i]]
    assert not bad, f"{len(bad)} answers differ from the recorded ones, first: {bad[:5]}"
    # tower form goes with the paired form, never without it
    assert all(p == "1" for p, t in zip(paired, tower) if t == "1")
    assert set(paired) == {"0", "1"} and set(tower) == {"0", "1"}
