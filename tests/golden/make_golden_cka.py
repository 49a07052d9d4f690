#!/usr/bin/env python3
"""Generate tests/golden/golden_cka.npz by running the REFERENCE's own utils/cka.py (get_linear_CKA, get_kernel_CKA) on the
seeded cases of tests/cka_oracle.py.  Run only where a checkout of the reference exists (never on the GPU box):

    python tests/golden/make_golden_cka.py <reference checkout>

The reference is fed the fp32 inputs widened to fp64 (the engine must match what it computes in exact arithmetic); the
bandwidth is the one its own rbf picks.  The file stores the case list (kind, seed, n, p, sigma) and the results only."""
import importlib.util
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import cka_oracle as O  # noqa: E402


def main(ref_root):
    spec = importlib.util.spec_from_file_location('ref_cka', os.path.join(ref_root, 'utils', 'cka.py'))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    rows = []
    for kind, seed, n, p, sigma in O.CASES:
        x, y = O.make_case(kind, seed, n, p)
        X, Y = x.astype(np.float64), y.astype(np.float64)
        s = sigma if sigma > 0 else None
        lin = R.get_linear_CKA(X, Y)
        ker = R.get_kernel_CKA(X, Y, s)
        if s is None:
            sx, sy = (_ref_sigma(R, M) for M in (X, Y))
        else:
            sx = sy = s
        rows.append((lin, ker, sx, sy))
        print(kind, seed, n, p, sigma, rows[-1], flush=True)
    np.savez(os.path.join(HERE, 'golden_cka.npz'),
             kind=np.array([c[0] for c in O.CASES]), seed=np.array([c[1] for c in O.CASES], dtype=np.int64),
             n=np.array([c[2] for c in O.CASES], dtype=np.int64), p=np.array([c[3] for c in O.CASES], dtype=np.int64),
             sigma=np.array([c[4] for c in O.CASES]), result=np.array(rows, dtype=np.float64))


def _ref_sigma(R, M):
    """The bandwidth the reference's rbf picks for M (utils/cka.py:22-24), captured at its math.sqrt call."""
    seen = []

    class _Math:
        @staticmethod
        def sqrt(v):
            seen.append(float(v))
            return math.sqrt(v)

    real, R.math = R.math, _Math
    try:
        R.rbf(M)
    finally:
        R.math = real
    return math.sqrt(seen[-1])


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
