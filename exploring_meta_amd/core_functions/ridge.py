"""The differentiable ridge-regression head of R2-D2 (Bertinetto et al., "Meta-learning with differentiable closed-form solvers") on the
4-conv trunk: the head's own inner problem, under a squared loss, solved to optimality on the support set -- the limit of ANIL's inner
loop -- through one fused HIP call (mi_meta_batch_ridge: the ANIL call's trunk pass, one ridge-head launch that builds, factorises and
differentiates through every task's Gram system, the trunk backward).  Per task, with the support / query features fs / fq:

    A = (fs fs^T + lam I)^-1 onehot(ys)        logits = scale * (fq fs^T) A

``lam`` (the regulariser) and ``scale`` (the logit scale) are the head's two hyper-parameters, meta-learned by default (``RidgeHead``).
R2-D2's additive logit bias is left out: under softmax cross-entropy its gradient is identically zero.  ``features`` is what the ANIL
entries take, and the engine is the ANIL one: a trunk trained with ``vision.anil_vision`` is scored here as it is."""
import math

import torch

from ..engine import check_ridge
from .metric import _closed_form_adapt, _fast_adapt, _score_test_tasks


class RidgeHead(torch.nn.Module):
    """The ridge head's two scalars, held as ``log_lam`` and ``log_scale``: positivity needs no clamping, and the chain rule
    (dlam * lam, dscale * scale) is applied in the fused call's autograd Function (metric._FusedClosedForm).  learnable=False: buffers, no parameters."""

    def __init__(self, lam=1.0, scale=1.0, learnable=True):
        super().__init__()
        lam, scale = check_ridge(lam, scale)
        self.learnable = bool(learnable)
        for name, v in (('log_lam', lam), ('log_scale', scale)):
            t = torch.tensor(math.log(v), dtype=torch.float32)
            if self.learnable:
                setattr(self, name, torch.nn.Parameter(t))
            else:
                self.register_buffer(name, t)

    @property
    def lam(self):
        return float(torch.exp(self.log_lam.detach().double()))

    @property
    def scale(self):
        return float(torch.exp(self.log_scale.detach().double()))

    def extra_repr(self):
        return f'lam={self.lam:.6g}, scale={self.scale:.6g}, learnable={self.learnable}'


def meta_batch_adapt_ridge(features, head, data, labels, shots, ways):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU, head a ``RidgeHead`` -> (loss_sum, loss[T], acc[T]).
    ``loss_sum.backward()`` fills ``.grad`` of the trunk's parameters and of the head's two (the sum of the per-task rows); under
    ``torch.no_grad()`` the call only scores.  loss and acc are plain values, as in ``meta_batch_adapt_metric``."""
    if not isinstance(head, RidgeHead):
        raise TypeError(f'head must be a RidgeHead, got {type(head).__name__}')
    lam, scale = check_ridge(head.lam, head.scale)
    return _closed_form_adapt('ridge', features, data, labels, shots, ways, dict(lam=lam, scale=scale), (head.log_lam, head.log_scale))


def fast_adapt_ridge(batch, features, head, shots, ways, device):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    return _fast_adapt(batch, device, lambda d, l: meta_batch_adapt_ridge(features, head, d, l, shots, ways))


def evaluate_ridge(params, test_tasks, features, head, device):
    """The counterpart of ``evaluate`` with the exactly solved head: the mean query accuracy of params['meta_batch_size'] test tasks,
    sampled in ``evaluate``'s order, from ONE batched call without a gradient.  ``features`` as for ``evaluate_nil``."""
    if not isinstance(head, RidgeHead):
        raise TypeError(f'head must be a RidgeHead, got {type(head).__name__}')
    check_ridge(head.lam, head.scale)
    ridge_test_accuracy = _score_test_tasks(params, test_tasks, features, device, lambda base, d, l: meta_batch_adapt_ridge(
        base, head, d, l, params['shots'], params['ways']))
    print('Ridge Test Accuracy', ridge_test_accuracy)
    return ridge_test_accuracy
