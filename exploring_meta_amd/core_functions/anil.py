"""ANIL through the reference's own call: ``fast_adapt(batch, learner, loss, K, shots, ways, device, features=features)``
with ``features = Sequential(ConvBase, Lambda(view(-1, fc_neurons)))`` and ``learner = MAML(Linear(fc_neurons, ways)).clone()``
(reference vision/anil_vision.py:86-94,116-122).  The fused HIP call runs the trunk once on all rows, adapts the head, and
returns a loss whose ``.backward()`` fills ``.grad`` of both the trunk's and the head's parameters."""
import torch

from ..engine import MetaEngine, ModelSpec
from .maml import MAML
from .vision import flat_theta, split_grad
from .vision_models import ConvBase

_engines = {}


def _find_convbase(features):
    if isinstance(features, ConvBase):
        return features
    for m in features.modules():
        if isinstance(m, ConvBase):
            return m
    raise ValueError('features must contain an exploring_meta_amd ConvBase trunk (reference anil_vision.py:86-91)')


class _FusedAnil(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, *params):
        loss, acc, grad, _ = engine.meta_batch_anil(flat_theta(params), data, labels, shots, steps, lr, first_order=first_order,
                                                    with_grad=need_grad)
        ctx.shapes = [p.shape for p in params]
        ctx.save_for_backward(grad if grad is not None else torch.empty(0, device=data.device))
        # Only the SUM carries the meta-gradient (the engine reduces over tasks inside the fused call): the per-task losses are
        # values, so `losses.mean().backward()` fails loudly instead of stepping on zeros.
        ctx.mark_non_differentiable(loss, acc)
        return loss.sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        (grad,) = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('fast_adapt was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 8 + split_grad(grad, ctx.shapes, gsum)


def anil_engine(features, ways, in_h, device):
    """The MetaEngine (one per architecture and device) that runs `features` + a `ways`-way linear head on in_h x in_h images."""
    base = _find_convbase(features)
    spec = ModelSpec.anil(ways, base.hidden, base.channels, base.max_pool, base.layers, in_h)
    device = torch.device(device)
    key = (spec, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _engines:
        _engines[key] = MetaEngine(spec, device)
    return _engines[key]


class _FusedAnilLR(torch.autograd.Function):
    """``_FusedAnil`` through mi_meta_batch_anil_lr: ``lr_flat`` [steps, Ph] (the head's step sizes, ``MAML.lr_flat()``) is one more
    differentiable input, so ``.backward()`` also carries lr_grad to a learnable ``InnerLR``'s values."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, first_order, need_grad, need_lr_grad, lr_flat, *params):
        lr_vec = lr_flat.detach().float().contiguous()
        if lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        loss, acc, grad, lr_grad, _ = engine.meta_batch_anil_lr(flat_theta(params), data, labels, shots, steps, lr_vec, first_order=first_order,
                                                                with_grad=need_grad, want_lr_grad=need_grad and need_lr_grad)
        ctx.shapes = [p.shape for p in params]
        empty = torch.empty(0, device=data.device)
        ctx.save_for_backward(grad if grad is not None else empty, lr_grad if lr_grad is not None else empty)
        ctx.mark_non_differentiable(loss, acc)
        return loss.sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('fast_adapt was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 8 + (lr_grad * gsum if lr_grad.numel() else None,) + split_grad(grad, ctx.shapes, gsum)


class _FusedAnilSteps(torch.autograd.Function):
    """mi_meta_batch_anil_steps: the query loss and accuracy after every head step, and the multi-step loss
    J = sum_t sum_j w_j L_query,t(theta_j) as the value that carries the gradients.  ``step_w`` [steps] lives on the device; ``lr`` is the
    number, or ``lr_flat`` [steps, Ph] an input of the function."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, need_lr_grad, step_w, lr_flat, *params):
        lr_vec = None if lr_flat is None else lr_flat.detach().float().contiguous()
        if lr_vec is not None and lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        loss, acc, grad, lr_grad, _ = engine.meta_batch_anil_steps(flat_theta(params), data, labels, shots, steps, step_w,
                                                                   inner_lr=lr if lr_vec is None else None, lr_vec=lr_vec, first_order=first_order,
                                                                   with_grad=need_grad, want_lr_grad=need_grad and need_lr_grad)
        ctx.shapes = [p.shape for p in params]
        empty = torch.empty(0, device=data.device)
        ctx.save_for_backward(grad if grad is not None else empty, lr_grad if lr_grad is not None else empty)
        ctx.mark_non_differentiable(loss, acc)       # (values: only the objective carries the gradients)
        return (step_w.unsqueeze(1) * loss[1:]).sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('meta_batch_adapt_anil_steps was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 10 + (lr_grad * gsum if lr_grad.numel() else None,) + split_grad(grad, ctx.shapes, gsum)


def _anil_call_args(learner, features, data, ways):
    """What every batched ANIL entry needs: (engine, head, parameters in the reference's optimizer order, first order?, lr_flat or None)."""
    head = learner.module if isinstance(learner, MAML) else learner
    if isinstance(learner, MAML) and learner.offsets_flat() is not None:
        raise NotImplementedError('per-step offsets are implemented for the fused MAML vision call, not for the ANIL head')
    if not isinstance(head, torch.nn.Linear) or head.out_features != ways:
        raise ValueError('ANIL learner must wrap torch.nn.Linear(fc_neurons, ways) (reference anil_vision.py:93)')
    base = _find_convbase(features)
    _, _, c, h, w = data.shape
    engine = anil_engine(features, ways, h, data.device)
    params = list(base.parameters()) + [head.weight, head.bias]          # reference optimizer order (anil_vision.py:97)
    if head.in_features * ways + ways + sum(p.numel() for p in base.parameters()) != engine.param_count:
        raise ValueError(f'head.in_features={head.in_features} does not match the trunk output for {h}x{w} inputs')
    fo = learner.first_order if isinstance(learner, MAML) else False
    # step sizes per head parameter (an InnerLR, or allow_nograd with a frozen weight / bias): the vector call
    lr_flat = learner.lr_flat() if isinstance(learner, MAML) else None
    return engine, params, fo, lr_flat


def meta_batch_adapt_anil(learner, features, data, labels, adaptation_steps, shots, ways):
    """Batched ANIL entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU -> (loss_sum, loss[T], acc[T]).  A learner whose ``lr``
    is an ``InnerLR`` (or that freezes ``weight`` / ``bias`` under ``allow_nograd``) takes mi_meta_batch_anil_lr, and ``.backward()`` fills
    a learnable ``InnerLR``'s ``values.grad`` beside the trunk's and the head's."""
    engine, params, fo, lr_flat = _anil_call_args(learner, features, data, ways)
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    data, labels = data.float().contiguous(), labels.contiguous()
    if lr_flat is None:
        return _FusedAnil.apply(engine, data, labels, shots, adaptation_steps, learner.lr, fo, need, *params)
    need_lr = torch.is_grad_enabled() and lr_flat.requires_grad
    return _FusedAnilLR.apply(engine, data, labels, shots, adaptation_steps, fo, need or need_lr, need_lr, lr_flat, *params)


def meta_batch_adapt_anil_steps(learner, features, data, labels, adaptation_steps, shots, ways, step_weights=None, first_order=None):
    """``meta_batch_adapt_anil`` with the query set scored after 0, 1, .., adaptation_steps head steps in the one fused call (the trunk
    still runs once), and the multi-step loss as the outer objective: the semantics of ``meta_batch_adapt_steps``.  ``step_weights``: the K
    weights w_1 .. w_K (``msl_weights``; a list, or an fp32 tensor already on the device, which a caller may anneal in place); None:
    (0, .., 0, 1), the final loss only.  Returns (objective, losses [K + 1, T], accs [K + 1, T]); ``objective.backward()`` fills the
    trunk's, the head's and a learnable ``InnerLR``'s ``.grad``; under ``torch.no_grad()`` the call scores only."""
    engine, params, fo, lr_flat = _anil_call_args(learner, features, data, ways)
    if first_order is not None:
        fo = bool(first_order)
    K = int(adaptation_steps)
    if step_weights is None:
        step_weights = [0.0] * (K - 1) + [1.0]
    if not torch.is_tensor(step_weights):
        step_weights = torch.tensor([float(w) for w in step_weights], dtype=torch.float32, device=data.device)
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    need_lr = lr_flat is not None and torch.is_grad_enabled() and lr_flat.requires_grad
    return _FusedAnilSteps.apply(engine, data.float().contiguous(), labels.contiguous(), shots, K, learner.lr, fo, need or need_lr, need_lr,
                                 step_weights, lr_flat, *params)


def fast_adapt_anil(data, labels, learner, features, adaptation_steps, shots, ways):
    total, losses, accs = meta_batch_adapt_anil(learner, features, data.unsqueeze(0), labels.unsqueeze(0), adaptation_steps,
                                                shots, ways)
    return total, accs[0]
