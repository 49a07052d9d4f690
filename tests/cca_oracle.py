"""fp64 numpy restatement of the reference's CCA similarity (reference utils/cca.py:226-362), written from its six steps:

  1. covariance blocks Sxx, Sxy, Syy of the (neurons, datapoints) inputs (row means removed);
  2. Sxx /= max|Sxx|, Syy /= max|Syy|, Sxy /= sqrt(max|Sxx| max|Syy|);
  3. keep neuron i of X iff |Sxx_ii| >= epsilon (same for Y), crop; either side empty: every statistic is 0;
  4. add epsilon to both diagonals; inverse square roots V diag(f) V^T from eigh with THE PSEUDO-INVERSE RULE:
     f_i = 0 where |w_i| <= 1e-15 max|w|, |w_i|^(-1/2) elsewhere;
  5. s = singular values (descending) of Sxx^(-1/2) Sxy Syy^(-1/2);
  6. mean(s), sum(s), and the mean of s[:idx] with idx the first i in 0..len(s)-1 with sum(s[:i]) / sum(s) >= threshold
     (all of s if there is none).

Inputs here are [n, p] (rows = datapoints), the engine's layout; the two sides may have different widths.  Also the seeded cases
of tests/golden/golden_cca.npz."""
import numpy as np

import cka_oracle

EPSILONS = (1e-10, 1e-6, 0.0)


def _inv_sqrt(S):
    w, v = np.linalg.eigh(S)
    a = np.abs(w)
    cut = 1e-15 * a.max()
    f = np.zeros_like(a)
    f[a > cut] = a[a > cut] ** -0.5
    cond = np.inf if a.min() <= cut else a.max() / a.min()
    return (v * f) @ v.T, float(cond)


def threshold_index(s, threshold):
    total = s.sum()
    for i in range(len(s)):
        with np.errstate(invalid='ignore', divide='ignore'):
            if s[:i].sum() / total >= threshold:
                return i
    return len(s)


def cca(X, Y, epsilon=0.0, threshold=0.98):
    """X [n, px], Y [n, py] -> dict(coefs, mean, thresholded_mean, sum, count, x_idxs, y_idxs, kept_x, kept_y, cond_x, cond_y, idx)"""
    X, Y = np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    n = X.shape[0]
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    Sxx, Sxy, Syy = Xc.T @ Xc / (n - 1), Xc.T @ Yc / (n - 1), Yc.T @ Yc / (n - 1)
    xmax, ymax = np.abs(Sxx).max(), np.abs(Syy).max()
    with np.errstate(invalid='ignore', divide='ignore'):
        Sxx, Syy, Sxy = Sxx / xmax, Syy / ymax, Sxy / np.sqrt(xmax * ymax)
        x_idxs, y_idxs = np.abs(np.diagonal(Sxx)) >= epsilon, np.abs(np.diagonal(Syy)) >= epsilon
    kx, ky = int(x_idxs.sum()), int(y_idxs.sum())
    out = dict(x_idxs=x_idxs, y_idxs=y_idxs, kept_x=kx, kept_y=ky, count=min(kx, ky))
    if kx == 0 or ky == 0:
        out.update(coefs=np.zeros(0), mean=0.0, thresholded_mean=0.0, sum=0.0, cond_x=float('nan'), cond_y=float('nan'), idx=0)
        return out
    Sxx = Sxx[x_idxs][:, x_idxs] + epsilon * np.eye(kx)
    Syy = Syy[y_idxs][:, y_idxs] + epsilon * np.eye(ky)
    Sxy = Sxy[x_idxs][:, y_idxs]
    rx, cond_x = _inv_sqrt(Sxx)
    ry, cond_y = _inv_sqrt(Syy)
    s = np.abs(np.linalg.svd(rx @ Sxy @ ry, compute_uv=False))
    idx = threshold_index(s, threshold)
    out.update(coefs=s, mean=float(s.mean()), thresholded_mean=float(s[:idx].mean()) if idx else float('nan'), sum=float(s.sum()),
               cond_x=cond_x, cond_y=cond_y, idx=idx)
    return out


def partial_ratios(s):
    """sum(s[:i]) / sum(s) for i in 0..len(s)-1: what the threshold index is read from"""
    return np.array([s[:i].sum() / s.sum() for i in range(len(s))])


# ---- seeded cases (fp32 inputs; the golden file stores only the case table and the results)
def _base(kind, seed, n, p):
    return cka_oracle.make_case(kind, seed, n, p)


def make_case(kind, seed, n, p):
    """(X, Y) fp32 [n, p].  gauss / relu / rep: cka_oracle.make_case.  same: Y = X.  rot: Y = 3 X Q, Q orthogonal.  dead: relu with
    column 3 of X and columns 7, 8 of Y zeroed.  dupcol: column 5 of X := column 4.  lindep: column 5 := column 4 + column 2."""
    if kind in cka_oracle.KINDS:
        return _base(kind, seed, n, p)
    x, y = _base('relu', seed, n, p)
    x, y = x.copy(), y.copy()
    if kind == 'same':
        y = x.copy()
    elif kind == 'rot':
        q, _ = np.linalg.qr(_base('gauss', seed + 1000, p, p)[0].astype(np.float64))
        y = (3.0 * x.astype(np.float64) @ q).astype(np.float32)
    elif kind == 'dead':
        x[:, 3] = 0.0
        y[:, 7:9] = 0.0
    elif kind == 'dupcol':
        x[:, 5] = x[:, 4]
    elif kind == 'lindep':
        x[:, 5] = x[:, 4] + x[:, 2]
    else:
        raise ValueError(kind)
    return x, y


DEAD_X, DEAD_Y = [3], [7, 8]           # the columns the dead case zeroes

_SHAPES = [(k, s, n, p) for k, s, n, p, sigma in cka_oracle.CASES if p < n and p <= 64]
_SHAPES += [('rep', 40, 3200, 25), ('rep', 41, 20000, 25), ('gauss', 42, 800, 64), ('relu', 43, 3200, 64), ('gauss', 44, 300, 7),
            ('same', 21, 900, 25), ('rot', 21, 900, 25)]
CASES = [(k, s, n, p, eps) for k, s, n, p in _SHAPES for eps in EPSILONS]           # (kind, seed, n, p, epsilon)
CASES += [(k, 9, 800, 25, eps) for k in ('dead', 'dupcol', 'lindep') for eps in EPSILONS[:2]]
THRESHOLD = 0.98


def bar(cond_x, cond_y):
    """max(1e-9, 1024 cond 2^-53), cond from the golden file"""
    return max(1e-9, 1024.0 * max(cond_x, cond_y) * 2.0 ** -53)


# ---- cases at the limits of the domain mi_maml.h states (not in the golden file: CASES indexes it, this table does not)
LIMIT_CASES = [  # (kind, seed, n, p, epsilon, zeroed columns of X, zeroed columns of Y)
    ('relu', 60, 300, 63, 1e-10, (), ()),                   # odd p at the LDS maximum: the round-robin's padding player
    ('gauss', 61, 300, 64, 1e-10, (3,), (7, 8, 9)),         # p = 64 with odd kept counts 63 and 61
    ('gauss', 62, 200, 3, 1e-10, (1,), ()),                 # kept 2 x 3: the whitened block is wider than tall
    ('relu', 63, 200, 3, 1e-10, (), (1,)),                  # kept 3 x 2
    ('gauss', 64, 50, 1, 1e-10, (), ()),
    ('relu', 65, 50, 2, 0.0, (), ()),
    ('gauss', 66, 5, 25, 1e-6, (), ()),                     # n < p: both covariance blocks have rank 4, epsilon carries the rest
    ('relu', 67, 1025, 3, 1e-10, (), ()),                   # the first n with two row chunks
    ('gauss', 68, 70001, 3, 1e-10, (), ()),                 # past the cap of 64 row chunks
    ('relu', 69, 1 << 18, 2, 1e-10, (), ()),                # the largest n
]


def make_limit_case(kind, seed, n, p, zero_x=(), zero_y=()):
    x, y = (a.copy() for a in _base(kind, seed, n, p))
    x[:, list(zero_x)] = 0.0
    y[:, list(zero_y)] = 0.0
    return x, y


def thresholded(s, threshold):
    """(idx, mean of s[:idx]) by the reference's sum_threshold + np.mean (utils/cca.py:177-195,347-355): NaN for an empty prefix,
    which is what np.mean of an empty slice returns there."""
    idx = threshold_index(s, threshold)
    return idx, (float(s[:idx].mean()) if idx else float('nan'))


PAIR_CASES = [('gauss', 70 + k) if k % 2 == 0 else ('relu', 70 + k) for k in range(7)]       # the seven 3 x 2 pairs of the 70000-pair call
