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
from .anil import anil_engine
from .metric import _trunk_of
from .vision import flat_theta, split_grad


class RidgeHead(torch.nn.Module):
    """The ridge head's two scalars, held as ``log_lam`` and ``log_scale``: positivity needs no clamping, and the chain rule
    (dlam * lam, dscale * scale) is applied in the fused call's autograd Function.  learnable=False: buffers, no parameters."""

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


class _FusedRidge(torch.autograd.Function):
    """``_FusedMetric`` with the head's two scalars: ``params`` are (log_lam, log_scale, the trunk's parameters ...)."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, lam, scale, need_grad, log_lam, log_scale, *params):
        trunk = flat_theta(params)
        theta = torch.zeros(engine.param_count, dtype=torch.float32, device=trunk.device)
        theta[:trunk.numel()] = trunk
        loss, acc, grad, dhyper, _ = engine.meta_batch_ridge(theta, data, labels, shots, lam=lam, scale=scale, with_grad=need_grad)
        ctx.shapes = [p.shape for p in params]
        ctx.hyper = (lam, scale)
        if grad is not None:
            # the head's gradient: the sum of the per-task rows (one reduction of ours, in a fixed order)
            ctx.save_for_backward(grad[:trunk.numel()], dhyper.double().sum(dim=0))
        else:
            ctx.save_for_backward(torch.empty(0, device=data.device), torch.empty(0, device=data.device))
        # Only the SUM carries the meta-gradient, as in _FusedMetric
        ctx.mark_non_differentiable(loss, acc)
        return loss.sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, dh = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('meta_batch_adapt_ridge was run without gradients (torch.no_grad or no parameter requires grad)')
        lam, scale = ctx.hyper
        # d/dlog(x) = x d/dx
        dlog_lam = (dh[0] * lam).float() * gsum if ctx.needs_input_grad[7] else None
        dlog_scale = (dh[1] * scale).float() * gsum if ctx.needs_input_grad[8] else None
        return (None,) * 7 + (dlog_lam, dlog_scale) + split_grad(grad, ctx.shapes, gsum)


def meta_batch_adapt_ridge(features, head, data, labels, shots, ways):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU, head a ``RidgeHead`` -> (loss_sum, loss[T], acc[T]).
    ``loss_sum.backward()`` fills ``.grad`` of the trunk's parameters and of the head's two (the sum of the per-task rows); under
    ``torch.no_grad()`` the call only scores.  loss and acc are plain values, as in ``meta_batch_adapt_metric``."""
    if not isinstance(head, RidgeHead):
        raise TypeError(f'head must be a RidgeHead, got {type(head).__name__}')
    lam, scale = check_ridge(head.lam, head.scale)
    base = _trunk_of(features)
    engine = anil_engine(base, ways, data.shape[-2], data.device)
    params = list(base.parameters())
    hyper = (head.log_lam, head.log_scale)
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params + list(hyper))
    hyper = tuple(h.to(data.device) for h in hyper)
    return _FusedRidge.apply(engine, data.float().contiguous(), labels.contiguous(), shots, lam, scale, need, *hyper, *params)


def fast_adapt_ridge(batch, features, head, shots, ways, device):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    data, labels = batch
    total, _, accs = meta_batch_adapt_ridge(features, head, data.to(device).unsqueeze(0), labels.to(device).unsqueeze(0), shots, ways)
    return total, accs[0]


def evaluate_ridge(params, test_tasks, features, head, device):
    """The counterpart of ``evaluate`` with the exactly solved head: the mean query accuracy of params['meta_batch_size'] test tasks,
    sampled in ``evaluate``'s order, from ONE batched call without a gradient.  ``features`` as for ``evaluate_nil``."""
    if not isinstance(head, RidgeHead):
        raise TypeError(f'head must be a RidgeHead, got {type(head).__name__}')
    check_ridge(head.lam, head.scale)
    base = _trunk_of(features)
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        data = torch.stack([b[0] for b in batches]).to(device)
        labels = torch.stack([b[1] for b in batches]).to(device)
        data = data.reshape(data.shape[0], data.shape[1], base.channels, *data.shape[-2:])
        _, _, accs = meta_batch_adapt_ridge(base, head, data, labels, params['shots'], params['ways'])
        ridge_test_accuracy = accs.mean().item()
    print('Ridge Test Accuracy', ridge_test_accuracy)
    return ridge_test_accuracy
