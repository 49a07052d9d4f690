"""Linear and RBF-kernel CKA (reference utils/cka.py:9-60) on the GPU, without the reference's n x n Gram and centring matrices.

``cka`` is the batched call (one ``mi_cka`` launch sequence for many pairs); ``get_linear_CKA`` / ``get_kernel_CKA`` keep the
reference's names and signatures.  Rows are the points and columns the features, as in the reference (p <= 128 features,
2 <= n <= 2^18 points).  There is no CPU fallback: without a GPU these raise."""
from collections import namedtuple

import numpy as np
import torch

from .. import _lib

CkaResult = namedtuple('CkaResult', ['linear', 'kernel', 'sigma_x', 'sigma_y'])


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


def cka(xs, ys, sigma=None):
    """xs, ys: CUDA tensors [pairs, n, p] (or [n, p]).  Returns CkaResult of fp64 CUDA tensors [pairs]: linear CKA, RBF-kernel
    CKA and the bandwidths used for X and Y (``sigma`` given: that value for both; None: the median heuristic per matrix)."""
    xs, ys = _as_batch(xs, 'xs'), _as_batch(ys, 'ys')
    if xs.shape != ys.shape:
        raise ValueError(f'xs {tuple(xs.shape)} and ys {tuple(ys.shape)} differ')
    if xs.device != ys.device:
        raise ValueError('xs and ys are on different devices')
    pairs, n, p = xs.shape
    lib = _lib.load()
    with torch.cuda.device(xs.device):
        nbytes = lib.mi_cka_scratch_bytes(pairs, n, p)
        if nbytes == 0:
            raise ValueError(f'unsupported CKA shape: pairs={pairs}, n={n}, p={p} (1 <= p <= 128, 2 <= n <= 2^18)')
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=xs.device)
        out = torch.empty(pairs, 4, dtype=torch.float64, device=xs.device)
        s = float(sigma) if sigma is not None else 0.0
        if sigma is not None and not s > 0.0:
            raise ValueError('sigma must be positive')
        stream = torch.cuda.current_stream(xs.device).cuda_stream
        _lib.check(lib.mi_cka(stream, xs.data_ptr(), ys.data_ptr(), pairs, n, p, s, scratch.data_ptr(), nbytes, out.data_ptr()))
    return CkaResult(out[:, 0], out[:, 1], out[:, 2], out[:, 3])


def _device_matrix(a):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not torch.is_tensor(a):
        a = torch.as_tensor(a)
    if not a.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError('CKA runs on the GPU only (there is no CPU fallback) and no GPU is available')
        a = a.to(torch.device('cuda', torch.cuda.current_device()))
    if a.dim() != 2:
        raise ValueError(f'expected an [n, p] matrix, got {tuple(a.shape)}')
    return a


def get_linear_CKA(X, Y):
    """Reference utils/cka.py:40-45: HSIC_lin(X, Y) / sqrt(HSIC_lin(X, X) HSIC_lin(Y, Y)) as a Python float."""
    return float(cka(_device_matrix(X), _device_matrix(Y)).linear[0])


def get_kernel_CKA(X, Y, sigma=None):
    """Reference utils/cka.py:48-53: RBF-kernel CKA (median-distance bandwidth per matrix when sigma is None) as a Python float."""
    return float(cka(_device_matrix(X), _device_matrix(Y), sigma).kernel[0])
