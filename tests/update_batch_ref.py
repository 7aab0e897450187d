"""Helpers for the tests of the delta update's window / batch form
(rs16_update_device_batch, rs16_update_batch.hip).  TEST
INFRASTRUCTURE, like update_ref.py, whose references these tests use.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

from rs16._lib import lib

BatchConsts = namedtuple("BatchConsts", "quads_per_lane nslab rows_per_wave stripes_per_wave waves blocks")


def batch_consts(rows, width, n, nstripes):
    """rs16_host_update_batch_consts: the shape of the launch
    rs16_update_device_batch makes for `rows` rows of a window of `width` bytes,
    n deltas and nstripes stripes, or None."""
    out = (C.c_uint32 * 6)()
    ok = lib().rs16_host_update_batch_consts(rows, width, n, nstripes, out)
    return BatchConsts(*[int(v) for v in out]) if ok else None
