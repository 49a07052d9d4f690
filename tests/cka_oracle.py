"""fp64 restatement of linear and RBF-kernel CKA (reference utils/cka.py:9-60), written from the formulas, streamed in row blocks
so that no n x n matrix is held (n up to ~14k on the host):

  linear:  HSIC_lin(X, Y) = ||Xc^T Yc||_F^2,  Xc = X - column means;   CKA = HSIC(X, Y) / sqrt(HSIC(X, X) HSIC(Y, Y))
  kernel:  D_ij = ||x_i - x_j||^2 by direct differences;  sigma^2 = median{D_ij : i < j, D_ij != 0} (numpy's median: the mean of
           the two middle values of an even count) unless sigma is given;  K = exp(-D / (2 sigma^2));
           C_ij = K_ij - r_i/n - r_j/n + s/n^2 (r = row sums of K, s = their sum);  HSIC = sum_ij Cx_ij Cy_ij.

Also the seeded cases of tests/golden/golden_cka.npz (inputs from the hash generator of exploring_meta_amd/utils/synthetic.py)."""
import numpy as np
import torch

from exploring_meta_amd.utils import synthetic

BLOCK = 512


def _sqdist(A, B):
    """[len(A), len(B)] squared distances by direct differences (fp64): exactly 0 iff the rows are equal."""
    return torch.cdist(A, B, compute_mode='donot_use_mm_for_euclid_dist') ** 2


def _t(X):
    return torch.as_tensor(np.asarray(X, dtype=np.float64))


def median_sigma2(X):
    X = _t(X)
    n = X.shape[0]
    vals = []
    for i0 in range(0, n, BLOCK):
        d = _sqdist(X[i0:i0 + BLOCK], X)
        rows = torch.arange(i0, min(i0 + BLOCK, n)).unsqueeze(1)
        d = d[torch.arange(n).unsqueeze(0) > rows]            # upper triangle, i < j
        vals.append(d[d != 0].numpy())
    v = np.concatenate(vals)
    if v.size == 0:
        return float('nan')
    k0, k1 = (v.size - 1) // 2, v.size // 2
    v.partition([k0, k1])
    return 0.5 * (v[k0] + v[k1])


def _kernel_rows(X, sig2, i0):
    return torch.exp(-_sqdist(X[i0:i0 + BLOCK], X) / (2.0 * sig2))


def kernel_cka(X, Y, sigma=None):
    """-> (kernel CKA, sigma_x, sigma_y)"""
    X, Y = _t(X), _t(Y)
    n = X.shape[0]
    if sigma is None:
        sx2, sy2 = median_sigma2(X), median_sigma2(Y)
    else:
        sx2 = sy2 = float(sigma) ** 2
    cs = []
    for M, s2 in ((X, sx2), (Y, sy2)):
        r = torch.cat([_kernel_rows(M, s2, i0).sum(1) for i0 in range(0, n, BLOCK)])
        cs.append(r / n - r.sum() / (2.0 * n * n))
    cx, cy = cs
    hxy = hxx = hyy = 0.0
    for i0 in range(0, n, BLOCK):
        i1 = min(i0 + BLOCK, n)
        Cx = _kernel_rows(X, sx2, i0) - cx[i0:i1, None] - cx[None, :]
        Cy = _kernel_rows(Y, sy2, i0) - cy[i0:i1, None] - cy[None, :]
        hxy += float((Cx * Cy).sum())
        hxx += float((Cx * Cx).sum())
        hyy += float((Cy * Cy).sum())
    return hxy / np.sqrt(hxx * hyy), float(np.sqrt(sx2)), float(np.sqrt(sy2))


def linear_cka(X, Y):
    X, Y = _t(X), _t(Y)
    Xc, Yc = X - X.mean(0), Y - Y.mean(0)
    h = lambda A, B: float(((A.T @ B) ** 2).sum())      # noqa: E731
    return h(Xc, Yc) / np.sqrt(h(Xc, Xc) * h(Yc, Yc))


def cka(X, Y, sigma=None):
    k, sx, sy = kernel_cka(X, Y, sigma)
    return dict(linear=linear_cka(X, Y), kernel=k, sigma_x=sx, sigma_y=sy)


# ---- seeded cases (fp32 inputs; the golden file stores only kind, seed, shape and sigma)
KINDS = ('gauss', 'relu', 'rep')


def make_case(kind, seed, n, p):
    """(X, Y) fp32 [n, p].  gauss: Gaussian-like rows, Y a noisy linear map of X.  relu: ReLU-sparse rows with all-zero rows and
    duplicated rows (what max-pooled ReLU reps look like).  rep: a [p, c, h, w] rep-shaped tensor (c*h*w = n) under the
    rc_vision reshape (c*h*w, b)."""
    if kind == 'rep':
        c = n // 25
        x4 = np.maximum(synthetic.hash_normalish(seed, (p, c, 5, 5), 0), 0.0)
        y4 = np.maximum(x4 + 0.5 * synthetic.hash_normalish(seed, (p, c, 5, 5), 1), 0.0)
        return x4.astype(np.float32).reshape(n, p), y4.astype(np.float32).reshape(n, p)
    x = synthetic.hash_normalish(seed, (n, p), 0)
    w = synthetic.hash_normalish(seed, (p, p), 2) / np.sqrt(p)
    y = x @ w + 0.5 * synthetic.hash_normalish(seed, (n, p), 1)
    if kind == 'relu':
        x, y = np.maximum(x - 0.3, 0.0), np.maximum(y - 0.3, 0.0)
        nz = max(1, n // 12)
        x[:nz] = 0.0                                        # all-zero rows
        y[n // 2:n // 2 + nz] = 0.0
        nd = max(1, n // 60)
        x[n - nd:] = x[nz:nz + nd]                          # duplicated rows
        y[n - nd:] = y[:nd]
    return x.astype(np.float32), y.astype(np.float32)


CASES = [  # (kind, seed, n, p, sigma or 0 = median)
    ('gauss', 1, 5, 1, 0.0), ('gauss', 2, 5, 25, 0.0), ('gauss', 3, 200, 5, 0.0), ('gauss', 4, 200, 100, 0.0),
    ('gauss', 5, 800, 25, 0.0), ('gauss', 6, 3200, 25, 0.0), ('gauss', 7, 800, 1, 0.0),
    ('relu', 8, 200, 5, 0.0), ('relu', 9, 800, 25, 0.0), ('relu', 10, 3200, 25, 0.0), ('relu', 11, 200, 100, 0.0),
    ('rep', 12, 800, 25, 0.0),
    ('gauss', 13, 200, 5, 2.5), ('relu', 14, 800, 25, 1.5),
]


# ---- cases at the limits of the domain mi_maml.h states (not in the golden file: CASES indexes it, this table does not)
LIMIT_SHAPES = [  # (n, p): p at and beside the maximum, the histogram's 64 KiB LDS crossing (512 p + 16384 bytes: p = 96 -> 97), the
    # smallest n, the 64-row tile edge, the first column split of the symmetric passes (n = 1025: S = 2) and its next tile count
    (130, 128), (130, 127), (70, 97), (70, 96), (2, 3), (3, 1), (63, 4), (64, 4), (65, 4), (1025, 3), (2049, 2),
]
_RELU_SEED = {(3, 1): 59}      # relu rows [0, a, a] / [b, 0, b] with a, b > 0 (most seeds clip a or b to 0: every output NaN)
LIMIT_CASES = [(kind, _RELU_SEED.get((n, p), 50 + i) if kind == 'relu' else 50 + i, n, p, 0.0)
               for i, (n, p) in enumerate(LIMIT_SHAPES) for kind in ('gauss', 'relu')]
LIMIT_CASES += [('gauss', 50, 130, 128, 2.0), ('relu', 50, 130, 128, 2.0)]            # (kind, seed, n, p, sigma or 0 = median)


def nonzero_sqdists(X):
    """The nonzero squared distances of the rows i < j, sorted: sum_k (x_ik - x_jk)^2 in fp64 without the square root that _sqdist
    takes and squares again (cdist gives 5.000000000000001 for the lattice distance 5), so integer inputs give exact integers.
    Holds an [n, n, p] array: small inputs only."""
    X = np.asarray(X, dtype=np.float64)
    d = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)[np.triu_indices(X.shape[0], 1)]
    return np.sort(d[d != 0])


def middle_ranks(X):
    """(count, value at rank (count - 1) // 2, value at rank count // 2) of the nonzero squared distances: the median is their mean."""
    v = nonzero_sqdists(X)
    return v.size, float(v[(v.size - 1) // 2]), float(v[v.size // 2])


def lattice_rows(seed, n, dup=None):
    """fp32 [n, 2] rows on the integer lattice {0..3}^2 (every squared distance an exact small integer, heavily tied); dup = (i, j):
    row i := row j."""
    x = np.floor(synthetic.hash_uniform(seed, (n, 2)) * 4.0).astype(np.float32)
    if dup is not None:
        x[dup[0]] = x[dup[1]]
    return x


TIE_CASES = [  # (seed of X, seed of Y, n, dup): n = 40, and n = 41 with row 40 a copy of row 7.  The X of the last two has an even
    # count of nonzero distances whose two middle ranks are 4 and 5 (tests/test_cka_host.py checks it): sigma^2 = 4.5
    (1, 2, 40, None), (3, 4, 41, (40, 7)), (359, 6, 40, None), (332, 8, 41, (40, 7)),
]


def exact_median_sigma2(X):
    """numpy's median of the nonzero squared distances from nonzero_sqdists: exact on lattice inputs"""
    count, lo, hi = middle_ranks(X)
    return 0.5 * (lo + hi)
