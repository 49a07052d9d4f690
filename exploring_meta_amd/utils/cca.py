"""CCA similarity of layer representations (reference utils/cca.py:226-362) on the GPU: the measure the reference's
representation-change study runs (``get_cca_similarity(adapted_rep.T, init_rep.T, epsilon=1e-10)[1]``).

``cca`` is the batched call (one ``mi_cca`` launch sequence for many pairs, rows = datapoints, columns = neurons, the engine's
layout); ``get_cca_similarity`` keeps the reference's name, (neurons, datapoints) orientation and ``(dict, float)`` return.
1 <= p <= 64 neurons on both sides, 2 <= n <= 2^18 datapoints.  There is no CPU fallback: without a GPU these raise.

One deliberate difference from the reference: a singular covariance block with ``epsilon = 0`` (dead or linearly dependent
neurons).  The reference's outcome there is an accident of rounding (typically ``LinAlgError``, its ``sqrt`` meeting an
eigenvalue of -1e-17); here the pseudo-inverse rule is stated once (an eigenvalue with ``|w_i| <= 1e-15 max|w|`` contributes 0,
every other one ``|w_i|^(-1/2)``) and gives a finite value: a cut direction adds a zero coefficient.  When either side keeps no
neuron (a constant matrix, for every epsilon) every statistic is 0 and every coefficient NaN, which is what the reference's
``create_zero_dict`` intends."""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib

CcaResult = namedtuple('CcaResult', ['coefs', 'mean', 'thresholded_mean', 'sum', 'count', 'kept_x', 'kept_y', 'cond_x', 'cond_y'])
CcaDetail = namedtuple('CcaDetail', ['x_mask', 'y_mask', 'sweeps'])


def _as_batch(a, name):
    if not torch.is_tensor(a):
        raise TypeError(f'{name} must be a torch tensor')
    if not a.is_cuda:
        raise RuntimeError(f'{name} must be a CUDA tensor (there is no CPU fallback)')
    if a.dim() == 2:
        a = a.unsqueeze(0)
    if a.dim() != 3:
        raise ValueError(f'{name} must be [pairs, n, p] or [n, p], got {tuple(a.shape)}')
    return a.to(torch.float32).contiguous()


def cca(xs, ys, epsilon=0.0, threshold=0.98, detail=False):
    """xs, ys: CUDA tensors [pairs, n, p] (or [n, p]).  Returns CcaResult of fp64 CUDA tensors: ``coefs`` [pairs, p] (the canonical
    correlations, descending, NaN after ``count``) and [pairs] each of the mean, the thresholded mean, the sum, count, the neurons
    kept on each side and the condition numbers of the two blocks as they enter the inverse (inf if the pseudo-inverse rule cuts
    the smallest eigenvalue).  ``detail=True`` also returns CcaDetail: the kept masks (int64 [pairs], bit i = neuron i) and the
    Jacobi sweeps (int32 [pairs, 4]: X and Y eigen-problems, singular values, 1 if a sweep cap was reached)."""
    xs, ys = _as_batch(xs, 'xs'), _as_batch(ys, 'ys')
    if xs.shape != ys.shape:
        raise ValueError(f'xs {tuple(xs.shape)} and ys {tuple(ys.shape)} differ')
    if xs.device != ys.device:
        raise ValueError('xs and ys are on different devices')
    epsilon, threshold = float(epsilon), float(threshold)
    if not epsilon >= 0.0:
        raise ValueError('epsilon must be >= 0')
    if not 0.0 <= threshold <= 1.0:
        raise ValueError('threshold must be in [0, 1]')
    pairs, n, p = xs.shape
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        nbytes = lib.mi_cca_scratch_bytes(pairs, n, p)
        if nbytes == 0:
            raise ValueError(f'unsupported CCA shape: pairs={pairs}, n={n}, p={p} (1 <= p <= 64, 2 <= n <= 2^18)')
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=xs.device)
        coefs = torch.empty(pairs, p, dtype=torch.float64, device=xs.device)
        stats = torch.empty(pairs, 8, dtype=torch.float64, device=xs.device)
        stream = torch.cuda.current_stream(xs.device).cuda_stream
        _lib.check(lib.mi_cca(stream, xs.data_ptr(), ys.data_ptr(), pairs, n, p, epsilon, threshold, scratch.data_ptr(), nbytes,
                              coefs.data_ptr(), stats.data_ptr()))
    res = CcaResult(coefs, *(stats[:, k] for k in range(8)))
    if not detail:
        return res
    masks = scratch[:pairs * 16].view(torch.int64).reshape(pairs, 2).clone()
    off = (pairs * 16 + 255) // 256 * 256
    sweeps = scratch[off:off + pairs * 16].view(torch.int32).reshape(pairs, 4).clone()
    return res, CcaDetail(masks[:, 0], masks[:, 1], sweeps)


def _device_acts(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a):
        a = torch.as_tensor(a)
    if a.dim() != 2:
        raise ValueError(f'expected a (neurons, datapoints) matrix, got {tuple(a.shape)}')
    if not a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('CCA runs on the GPU only (there is no CPU fallback) and no GPU is available')
        a = a.to(torch.device('cuda', torch.cuda.current_device()))
    return a


def _mask_array(bits, p):
    bits = int(bits) & ((1 << 64) - 1)
    return np.array([(bits >> i) & 1 == 1 for i in range(p)], dtype=bool)


def _threshold_index(s, threshold):
    total = 0.0
    for v in s:
        total += v
    head = 0.0
    for i, v in enumerate(s):
        if total != 0.0 and head / total >= threshold:
            return i
        head += v
    return len(s)


def get_cca_similarity(acts1, acts2, epsilon=0., threshold=0.98, compute_coefs=True, compute_dirns=False, verbose=False):
    """Reference utils/cca.py:226-362.  acts1, acts2: (neurons, datapoints) numpy arrays or tensors (transposed on the device).
    Returns (dict, mean canonical correlation).  The dict has ``cca_coef1`` / ``cca_coef2`` (numpy, descending), ``mean`` and
    ``sum`` (pairs of equal values; ``mean`` is over the coefficients up to the threshold index), ``x_idxs`` / ``y_idxs``
    (boolean masks of the neurons kept) and ``idx1`` / ``idx2`` (the threshold index).  The neuron-coefficient matrices that
    ``compute_coefs`` adds in the reference (``coef_x``, ``invsqrt_xx``, ``full_coef_x``, ``full_invsqrt_xx``, their y twins,
    ``neuron_means1/2``) are not produced, and ``compute_dirns=True`` raises."""
    if compute_dirns:
        raise NotImplementedError('compute_dirns=True needs the neuron-coefficient matrices (coef_x, full_coef_x, full_invsqrt_xx and '
                                  'their y twins) and the CCA directions cca_dirns1 / cca_dirns2, which the GPU path does not produce')
    assert acts1.shape[1] == acts2.shape[1], "dimensions don't match"
    assert acts1.shape[0] < acts1.shape[1], 'input must be number of neurons by datapoints'
    if acts1.shape[0] != acts2.shape[0]:
        raise NotImplementedError('different neuron counts on the two sides are not supported')
    a1, a2 = _device_acts(acts1), _device_acts(acts2)
    res, det = cca(a1.t(), a2.t(), epsilon, threshold, detail=True)
    p = a1.shape[0]
    count = int(res.count[0])
    s = res.coefs[0, :count].cpu().numpy()
    idx = _threshold_index(s.tolist(), float(threshold)) if count else 0
    mean_t, total = float(res.thresholded_mean[0]), float(res.sum[0])
    out = {
        'cca_coef1': s, 'cca_coef2': s.copy(),
        'x_idxs': _mask_array(det.x_mask[0], p), 'y_idxs': _mask_array(det.y_mask[0], p),
        'mean': (mean_t, mean_t), 'sum': (total, total), 'idx1': idx, 'idx2': idx,
    }
    if verbose:
        print(f'cca: kept {int(res.kept_x[0])} / {int(res.kept_y[0])} neurons, cond {float(res.cond_x[0]):.3g} / {float(res.cond_y[0]):.3g}')
    return out, float(res.mean[0])
