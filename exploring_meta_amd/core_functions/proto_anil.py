"""Proto-MAML on the ANIL trunk (Triantafillou et al., "Meta-Dataset", eq. 8): ANIL's head inner loop started, per task, from the linear
head that reproduces the Prototypical-Networks logits on the support prototypes c_w,

    W_0[w] = 2 scale c_w        b_0[w] = -scale |c_w|^2

instead of from a learned initialisation, and differentiated through both the loop and the initialisation, through one fused HIP call
(mi_meta_batch_anil_proto: the ANIL call's launches plus the initialisation and its backward).  With no inner step it is Prototypical
Networks; with K steps it answers whether ANIL's learned head initialisation carries anything the features do not.  The learner
(``MAML(Linear(fc_neurons, ways), lr | InnerLR)``) supplies the step sizes and the order; its weight and bias enter no result and receive
zero gradients.  ``scale`` is meta-learned by default (``ProtoInit``).  The engine is the ANIL one: a trunk trained with
``vision.anil_vision`` is scored here as it is."""
import math

import torch

from .anil import _anil_call_args
from .metric import _fast_adapt, _trunk_of
from .vision import split_grad, flat_theta


class ProtoInit(torch.nn.Module):
    """The initialisation's one scalar, held as ``log_scale``: positivity needs no clamping, and the chain rule (dscale * scale) is applied
    in the fused call's autograd Function.  learnable=False: a buffer, no parameter."""

    def __init__(self, scale=1.0, learnable=True):
        super().__init__()
        scale = float(scale)
        if not (scale > 0.0 and math.isfinite(scale)):
            raise ValueError(f'the prototype initialisation\'s scale must be positive and finite, got {scale}')
        self.learnable = bool(learnable)
        t = torch.tensor(math.log(scale), dtype=torch.float32)
        if self.learnable:
            self.log_scale = torch.nn.Parameter(t)
        else:
            self.register_buffer('log_scale', t)

    @property
    def scale(self):
        return float(torch.exp(self.log_scale.detach().double()))

    def extra_repr(self):
        return f'scale={self.scale:.6g}, learnable={self.learnable}'


class _FusedProtoAnil(torch.autograd.Function):
    """mi_meta_batch_anil_proto.  ``step_w`` None: the plain outputs and the final loss as the objective; else the per-step outputs and
    the multi-step loss (``_FusedAnilSteps``).  ``lr`` is the number, or ``lr_flat`` [steps, Ph] an input of the function; ``log_scale``
    the tensor behind ``scale``."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, need_lr_grad, step_w, scale, log_scale, lr_flat, *params):
        lr_vec = None if lr_flat is None else lr_flat.detach().float().contiguous()
        if lr_vec is not None and lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        loss, acc, grad, lr_grad, dscale, _ = engine.meta_batch_anil_proto(
            flat_theta(params), data, labels, shots, steps, scale, inner_lr=lr if lr_vec is None else None, lr_vec=lr_vec, step_w=step_w,
            first_order=first_order, with_grad=need_grad, want_lr_grad=need_grad and need_lr_grad)
        ctx.shapes = [p.shape for p in params]
        ctx.scale = scale
        empty = torch.empty(0, device=data.device)
        # the scale's gradient: the sum of the per-task rows in fp64 (one reduction of ours, in a fixed order)
        ctx.save_for_backward(grad if grad is not None else empty, lr_grad if lr_grad is not None else empty,
                              dscale.double().sum() if dscale is not None else empty)
        ctx.mark_non_differentiable(loss, acc)       # (values: only the objective carries the gradients)
        return (loss.sum() if step_w is None else (step_w.unsqueeze(1) * loss[1:]).sum()), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad, dscale = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('meta_batch_adapt_proto_anil was run without gradients (torch.no_grad or no parameter requires grad)')
        dlog = (dscale * ctx.scale).float() * gsum if ctx.needs_input_grad[11] else None          # d/dlog(s) = s d/ds
        return (None,) * 11 + (dlog, lr_grad * gsum if lr_grad.numel() else None) + split_grad(grad, ctx.shapes, gsum)


def meta_batch_adapt_proto_anil(learner, features, init, data, labels, adaptation_steps, shots, ways, step_weights=None, first_order=None):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU, init a ``ProtoInit`` -> (objective, losses, accs).
    ``step_weights`` None: the objective is the sum of the tasks' query losses at theta_K, losses and accs are [T] (adaptation_steps = 0:
    Prototypical Networks).  ``step_weights`` (K weights, a list or an fp32 tensor on the device): the multi-step loss, losses and accs are
    [K + 1, T] with row 0 the Prototypical-Networks score.  ``objective.backward()`` fills ``.grad`` of the trunk's parameters, of
    ``init.log_scale`` and of a learnable ``InnerLR``'s values; the learner's weight and bias receive zeros.  Under ``torch.no_grad()``
    the call only scores."""
    if not isinstance(init, ProtoInit):
        raise TypeError(f'init must be a ProtoInit, got {type(init).__name__}')
    base = _trunk_of(features)
    engine, params, fo, lr_flat = _anil_call_args(learner, base, data, ways)
    if first_order is not None:
        fo = bool(first_order)
    K = int(adaptation_steps)
    if step_weights is not None and not torch.is_tensor(step_weights):
        step_weights = torch.tensor([float(w) for w in step_weights], dtype=torch.float32, device=data.device)
    log_scale = init.log_scale.to(data.device)
    need_lr = lr_flat is not None and torch.is_grad_enabled() and lr_flat.requires_grad
    need = torch.is_grad_enabled() and (any(p.requires_grad for p in params) or log_scale.requires_grad or need_lr)
    return _FusedProtoAnil.apply(engine, data.float().contiguous(), labels.contiguous(), shots, K, learner.lr, fo, need, need_lr, step_weights,
                                 init.scale, log_scale, lr_flat, *params)


def fast_adapt_proto_anil(batch, learner, features, init, adaptation_steps, shots, ways, device):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    return _fast_adapt(batch, device, lambda d, l: meta_batch_adapt_proto_anil(learner, features, init, d, l, adaptation_steps, shots, ways))


def evaluate_proto_anil(params, test_tasks, learner, features, init, device):
    """The counterpart of ``evaluate_steps``: the mean query accuracy of params['meta_batch_size'] test tasks, sampled in ``evaluate``'s
    order, after 0, 1, .., params['adapt_steps'] head steps from the prototype initialisation -- a list of K + 1 numbers from ONE batched
    call without a gradient.  Step 0 is Prototypical Networks' accuracy on the same tasks."""
    base = _trunk_of(features)
    K = int(params['adapt_steps'])
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        data = torch.stack([b[0] for b in batches]).to(device)
        labels = torch.stack([b[1] for b in batches]).to(device)
        data = data.reshape(data.shape[0], data.shape[1], base.channels, *data.shape[-2:])
        weights = [0.0] * (K - 1) + [1.0] if K >= 1 else None
        _, _, accs = meta_batch_adapt_proto_anil(learner, base, init, data, labels, K, params['shots'], params['ways'], step_weights=weights)
        per_step = [float(a) for a in accs.reshape(K + 1, -1).double().mean(dim=1)]
    print('Proto-ANIL Test Accuracy per step', per_step)
    return per_step
