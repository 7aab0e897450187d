#!/usr/bin/env python3
"""The encode decision on the CPU: rs16_host_verify_path over a grid of shapes.

With RS16_DIAG_FORCE_FUSED_VERIFY the hook returns EncodeForm::verify_fusable
itself, so two libraries that print the same listing decide the same encode
forms wherever a scrub can tell them apart.  Host arithmetic only: no GPU.

  RS16_LIB=<librs16.so> python scripts/sweep_verify_path.py > listing.txt

Prints one row per (k, m, S, nstripes, diag); the last line on stderr is the
row count and the SHA-256 of the listing (profiles/r21_encode_form_sweep.txt).
"""
import ctypes
import hashlib
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
LIB = os.environ.get("RS16_LIB", str(ROOT / "reed-solomon-16_amd" / "build" / "librs16.so"))

COUNTS = [1, 2, 3, 5, 33, 64, 100, 128, 129, 200, 256, 257, 300, 512, 513, 600, 1000, 1024, 1025, 2048, 3000, 4096,
          8000, 8192, 30000, 32768]
WIDTHS = [64, 192, 1024, 2048, 2112, 4096, 65536]
STRIPES = [1, 2, 4, 8, 64]
NO_COLUMN, FORCE_COLUMN, FORCE_FUSED = 8, 16, 65536  # (rs16.DIAG_*)
DIAGS = [FORCE_FUSED, FORCE_FUSED | NO_COLUMN, FORCE_FUSED | FORCE_COLUMN, 0, NO_COLUMN, FORCE_COLUMN]


def main():
    lib = ctypes.CDLL(LIB)
    sz = ctypes.c_size_t
    path = lib.rs16_host_verify_path
    path.restype, path.argtypes = ctypes.c_int, [sz, sz, sz, sz, ctypes.c_int]
    rows = []
    for k in COUNTS:
        for m in COUNTS:
            if path(k, m, 64, 1, 0) < 0:  # (the pair has no rate: k + m beyond the field)
                continue
            for S in WIDTHS:
                for n in STRIPES:
                    for d in DIAGS:
                        rows.append("%d:%d x %d, %d stripes, diag %d: %d" % (k, m, S, n, d, path(k, m, S, n, d)))
    text = "\n".join(rows) + "\n"
    sys.stdout.write(text)
    sys.stderr.write("%d rows, sha256 %s\n" % (len(rows), hashlib.sha256(text.encode()).hexdigest()))


if __name__ == "__main__":
    main()
