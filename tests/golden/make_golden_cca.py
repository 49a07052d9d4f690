#!/usr/bin/env python3
"""Generate tests/golden/golden_cca.npz by running the REFERENCE's own utils/cca.py (get_cca_similarity) on the seeded cases of
tests/cca_oracle.py.  Run only where a checkout of the reference exists (never on the GPU box):

    python tests/golden/make_golden_cca.py <reference checkout>

The reference is fed the fp32 inputs widened to fp64 and transposed to its (neurons, datapoints) orientation.  The file stores
the case table (kind, seed, n, p, epsilon) and, per case, the reference's coefficients (NaN-padded to p), mean, thresholded mean,
sum and both masks, plus the condition numbers of the two blocks as tests/cca_oracle.py computes them (the test bar is read from
those).  A case whose threshold index hinges on rounding (a partial ratio sum(s[:i]) / sum(s) within 1e-6 of the threshold) is
refused: change its seed."""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

import cca_oracle as O  # noqa: E402


def main(ref_root):
    spec = importlib.util.spec_from_file_location('ref_cca', os.path.join(ref_root, 'utils', 'cca.py'))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    pmax = max(c[3] for c in O.CASES)
    coefs = np.full((len(O.CASES), pmax), np.nan)
    stats = np.zeros((len(O.CASES), 5))                    # mean, thresholded mean, sum, cond_x, cond_y
    xm = np.zeros((len(O.CASES), pmax), dtype=bool)
    ym = np.zeros((len(O.CASES), pmax), dtype=bool)
    for idx, (kind, seed, n, p, eps) in enumerate(O.CASES):
        x, y = O.make_case(kind, seed, n, p)
        d, mean = R.get_cca_similarity(x.astype(np.float64).T, y.astype(np.float64).T, epsilon=eps, threshold=O.THRESHOLD)
        s = np.asarray(d['cca_coef1'], dtype=np.float64)
        ratios = O.partial_ratios(s)
        if np.any(np.abs(ratios - O.THRESHOLD) <= 1e-6):
            sys.exit(f'case {O.CASES[idx]}: a partial ratio is within 1e-6 of the threshold; change the seed')
        assert mean == np.mean(s) and d['mean'][0] == d['mean'][1] and d['sum'][0] == d['sum'][1]
        o = O.cca(x, y, eps, O.THRESHOLD)
        coefs[idx, :len(s)] = s
        stats[idx] = (mean, d['mean'][0], d['sum'][0], o['cond_x'], o['cond_y'])
        xm[idx, :p], ym[idx, :p] = d['x_idxs'], d['y_idxs']
        print(O.CASES[idx], 'mean', mean, 'cond', o['cond_x'], o['cond_y'], 'oracle err', np.abs(o['coefs'] - s).max(), flush=True)
    np.savez_compressed(os.path.join(HERE, 'golden_cca.npz'),
                        kind=np.array([c[0] for c in O.CASES]), seed=np.array([c[1] for c in O.CASES], dtype=np.int64),
                        n=np.array([c[2] for c in O.CASES], dtype=np.int64), p=np.array([c[3] for c in O.CASES], dtype=np.int64),
                        epsilon=np.array([c[4] for c in O.CASES]), threshold=np.array(O.THRESHOLD),
                        coefs=coefs, stats=stats, x_idxs=xm, y_idxs=ym)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
