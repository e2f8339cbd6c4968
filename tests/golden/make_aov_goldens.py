"""Generate tests/golden/aov/<name>.npz: the hit-record planes (include/rtx.h, rtx_aov_planes) of the
committed fuzz scenes of tests/golden/fuzz/ and of aov_ref.GOLDEN_EXTRA at 44 x 28, from the checker of
tests/aov_ref.py —
the oracle's own closest_hit (pinned to the reference by tests/test_fuzz_golden.py on these very
scenes) plus the id-tracking walk it is checked against.  Data only: depth and normal as float32,
material and primitive as uint32, flat and row-major.

Usage:  python tests/golden/make_aov_goldens.py
"""
from __future__ import annotations

import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import aov_ref  # noqa: E402
import checkers  # noqa: E402

W, H = aov_ref.GOLDEN_W, aov_ref.GOLDEN_H
OUT = HERE / "aov"


def main() -> None:
    OUT.mkdir(exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        lib = checkers.lib()
        for family, seed in aov_ref.golden_cases():
            name = f"{family}_{seed}"
            _keep, s, cam = aov_ref.golden_view(family, seed, td)
            p = aov_ref.planes(lib, s, cam, W, H)
            np.savez_compressed(OUT / f"{name}.npz", **p)
            kinds = np.bincount(aov_ref.kind(p["primitive"]), minlength=4)
            print(f"{name}: kinds none/sphere/plane/triangle = {kinds.tolist()}")


if __name__ == "__main__":
    main()
