"""Continual-learning metrics of a task-by-task result matrix (the reference's utils/cl_metrics.py; Diaz-Rodriguez et al., "Don't
forget, there is more than forgetting: new metrics for Continual Learning", 2018).  ``matrix[i, j]``: the score on task j of the learner
adapted on task i (misc_scripts/cl_vision.run_cl_exp, misc_scripts/cl_rl.run_cl_rl_exp)."""
import numpy as np


def calc_cl_metrics(matrix):
    """-> dict(av_acc, fwt, rem, bwt_plus) for an N x N matrix, N >= 2.

    av_acc    mean of the diagonal and everything below it: N (N + 1) / 2 entries
    fwt       forward transfer: mean of the entries above the diagonal, N (N - 1) / 2 of them
    bwt       (not returned) sum over rows i >= 1 and columns j <= N - 2 of matrix[i, j] - matrix[j, j], over N (N - 1) / 2
              -- the reference's sum, which takes every such column for every row, those right of the diagonal included
    rem       remembering, 1 - |min(bwt, 0)|: 1 when nothing was forgotten
    bwt_plus  max(bwt, 0): improvement on earlier tasks"""
    m = np.asarray(matrix, dtype=np.float64)
    if m.ndim != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 2:
        raise ValueError(f'calc_cl_metrics takes a square matrix of at least 2 x 2, got shape {m.shape}')
    n = m.shape[0]
    pairs = n * (n - 1) / 2
    lower = np.tril_indices(n)
    upper = np.triu_indices(n, 1)
    bwt = float((m[1:, :n - 1] - np.diag(m)[:n - 1]).sum() / pairs)
    return dict(av_acc=float(m[lower].sum() / (pairs + n)), fwt=float(m[upper].sum() / pairs), rem=1.0 - abs(min(bwt, 0.0)),
                bwt_plus=max(bwt, 0.0))
