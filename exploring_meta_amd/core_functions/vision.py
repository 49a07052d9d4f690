"""``fast_adapt`` / ``accuracy`` / ``evaluate`` with the reference's signatures (core_functions/vision.py:6-42), backed by
the batched HIP engine, plus the batched entry the engine is designed for (``meta_batch_adapt``)."""
import os

import torch

from .maml import MAML


def _check_loss(loss):
    if not isinstance(loss, torch.nn.CrossEntropyLoss) or loss.reduction != 'mean' or loss.weight is not None \
            or getattr(loss, 'label_smoothing', 0.0) != 0.0:
        raise ValueError("the HIP engine fuses torch.nn.CrossEntropyLoss(reduction='mean'), the loss every reference "
                         'vision script uses (maml_vision.py:86, anil_vision.py:99)')


# The meta-gradient is normally produced WITH the loss (one fused call).  A caller that adapts under enabled gradients but never
# calls backward -- the reference's validation half, maml_vision.py:117-124, which is not wrapped in no_grad -- then pays for an
# outer backward it discards (about 2/3 of a second-order call).  With this switch on (or MI_MAML_DEFERRED_BACKWARD=1) the forward
# runs the evaluation-only call and `backward` re-runs the fused call with the gradient: cheaper when fewer than about two thirds
# of the calls are followed by backward, dearer otherwise (the drivers here wrap validation in no_grad instead and leave it off).
DEFERRED_OUTER_BACKWARD = os.environ.get('MI_MAML_DEFERRED_BACKWARD', '0') == '1'


def flat_theta(params):
    """The parameters as the engine's theta: one flat fp32 vector in the given order."""
    return torch.cat([p.detach().reshape(-1) for p in params]).float().contiguous()


def split_grad(grad, shapes, scale):
    """The flat gradient times `scale`, back in the parameters' shapes."""
    outs, off = [], 0
    for shp in shapes:
        n = shp.numel()
        outs.append((grad[off:off + n] * scale).reshape(shp))
        off += n
    return tuple(outs)


class _FusedFastAdapt(torch.autograd.Function):
    """T tasks through mi_meta_batch_maml_tv, or mi_meta_batch_maml_lr when the step sizes come per parameter: ``lr`` is the number, or
    ``lr_flat`` [steps, P] an input of the function.  The meta-gradient is produced together with the loss (the outer backward is part
    of the fused call); ``backward`` hands it to autograd so ``eval_loss.backward()`` accumulates into ``.grad``, the step-size gradient
    next to it (``InnerLR.flat`` carries it to the stored values)."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, need_lr_grad, grad_tasks, lr_flat, *params):
        theta = flat_theta(params)
        lr_vec = None if lr_flat is None else lr_flat.detach().float().contiguous()
        if lr_vec is not None and lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        gt = data.shape[0] if grad_tasks is None else int(grad_tasks)

        def call(with_grad):
            """(loss, acc, grad, lr_grad) of the fused call, evaluation only or with the gradients."""
            if lr_vec is None:
                return engine.meta_batch(theta, data, labels, shots, steps, lr, first_order=first_order, grad_tasks=gt if with_grad else 0)[:3] + (None,)
            return engine.meta_batch_lr(theta, data, labels, shots, steps, lr_vec, first_order=first_order, grad_tasks=gt if with_grad else 0,
                                        want_lr_grad=with_grad and need_lr_grad)[:4]
        ctx.deferred = call if need_grad and DEFERRED_OUTER_BACKWARD else None
        loss, acc, grad, lr_grad = call(need_grad and ctx.deferred is None)
        ctx.shapes = [p.shape for p in params]
        empty = torch.empty(0, device=data.device)
        ctx.save_for_backward(grad if grad is not None else empty, lr_grad if lr_grad is not None else empty)
        # Only the SUM carries the meta-gradient (the engine reduces over tasks inside the fused call): the per-task losses are
        # values, so `losses.mean().backward()` fails loudly instead of stepping on zeros.
        ctx.mark_non_differentiable(loss, acc)
        return loss[:gt].sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad = ctx.saved_tensors
        if ctx.deferred is not None:
            _, _, grad, lr_grad = ctx.deferred(True)
            lr_grad = grad.new_empty(0) if lr_grad is None else lr_grad
        if grad.numel() == 0:
            raise RuntimeError('fast_adapt was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 10 + (lr_grad * gsum if lr_grad.numel() else None,) + split_grad(grad, ctx.shapes, gsum)


class _FusedFastAdaptOffsets(torch.autograd.Function):
    """``_FusedFastAdapt`` / ``_FusedFastAdaptSteps`` through mi_meta_batch_maml_offsets: per-step parameter offsets ``ofs_flat`` [steps, P]
    (``MAML.offsets_flat()``) are one more input of the function, and ``backward`` hands autograd their gradient beside the model's and the
    step sizes' (``StepOffsets.flat`` carries it to the stored values).  ``step_w`` None: the plain objective, the sum of the train tasks'
    final query losses; else the multi-step loss."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, need_lr_grad, need_ofs_grad, grad_tasks, step_w, lr_flat,
                ofs_flat, *params):
        theta = flat_theta(params)
        lr_vec = None if lr_flat is None else lr_flat.detach().float().contiguous()
        if lr_vec is not None and lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        if ofs_flat.shape[0] != int(steps):
            raise ValueError(f'the learner holds per-step offsets for {ofs_flat.shape[0]} inner steps, the call adapts for {steps}')
        offsets = ofs_flat.detach().float().contiguous()
        gt = data.shape[0] if grad_tasks is None else int(grad_tasks)

        def call(with_grad):
            """(loss, acc, grad, lr_grad, offsets_grad) of the fused call, evaluation only or with the gradients."""
            return engine.meta_batch_offsets(theta, data, labels, shots, steps, offsets, inner_lr=lr if lr_vec is None else None, lr_vec=lr_vec,
                                             step_w=step_w, first_order=first_order, grad_tasks=gt if with_grad else 0,
                                             want_lr_grad=with_grad and need_lr_grad and lr_vec is not None,
                                             want_offsets_grad=with_grad and need_ofs_grad)[:5]
        ctx.deferred = call if need_grad and DEFERRED_OUTER_BACKWARD else None
        loss, acc, grad, lr_grad, ofs_grad = call(need_grad and ctx.deferred is None)
        ctx.shapes = [p.shape for p in params]
        empty = torch.empty(0, device=data.device)
        ctx.save_for_backward(*(empty if t is None else t for t in (grad, lr_grad, ofs_grad)))
        ctx.mark_non_differentiable(loss, acc)       # (values: only the objective carries the gradients, as in _FusedFastAdapt)
        return (loss[:gt].sum() if step_w is None else (step_w.unsqueeze(1) * loss[1:, :gt]).sum()), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad, ofs_grad = ctx.saved_tensors
        if ctx.deferred is not None:
            _, _, grad, lr_grad, ofs_grad = ctx.deferred(True)
            lr_grad = grad.new_empty(0) if lr_grad is None else lr_grad
            ofs_grad = grad.new_empty(0) if ofs_grad is None else ofs_grad
        if grad.numel() == 0:
            raise RuntimeError('the fused call was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 12 + (lr_grad * gsum if lr_grad.numel() else None, ofs_grad * gsum if ofs_grad.numel() else None) + \
            split_grad(grad, ctx.shapes, gsum)


def _adapt_with_offsets(learner, model, data, labels, K, shots, fo, grad_tasks, step_w, ofs_flat):
    """The offsets call of ``meta_batch_adapt`` (step_w None) and ``meta_batch_adapt_steps``."""
    if not hasattr(model, 'spec') or not hasattr(model, 'engine'):
        raise NotImplementedError('per-step offsets are implemented for the fused MAML vision call')
    if ofs_flat.shape[0] != K:
        raise ValueError(f'the learner holds per-step offsets for {ofs_flat.shape[0]} inner steps, adaptation_steps is {K} '
                         '(StepOffsets(model, steps) must have one row per inner step)')
    params = list(model.parameters())
    ge = torch.is_grad_enabled()
    need = ge and any(p.requires_grad for p in params)
    lr_flat = learner.lr_flat()
    need_lr = lr_flat is not None and ge and lr_flat.requires_grad
    need_ofs = ge and ofs_flat.requires_grad
    return _FusedFastAdaptOffsets.apply(model.engine(), data, labels.contiguous(), shots, K, learner.lr, fo, need or need_lr or need_ofs, need_lr,
                                        need_ofs, grad_tasks, step_w, lr_flat, ofs_flat, *params)


def meta_batch_adapt(learner, data, labels, adaptation_steps, shots, ways, first_order=None, grad_tasks=None):
    """Batched entry: data [T, 2*shots*ways, C, H, W], labels [T, 2*shots*ways] on the GPU.
    Returns (loss_sum, loss[T], acc[T]); ``loss_sum.backward()`` accumulates the SUM over tasks of d valid_loss/d theta
    into the base parameters' ``.grad`` -- what T iterations of the reference loop body leave there.  ``loss[T]`` and ``acc[T]``
    are plain values (not differentiable): weight tasks by scaling ``loss_sum``, or call once per group of tasks.
    A learner with per-step offsets (``MAML(..., offsets=StepOffsets(...))``) takes mi_meta_batch_maml_offsets, and ``.backward()`` fills
    ``StepOffsets.values.grad`` too; its offsets must hold ``adaptation_steps`` rows.
    ``grad_tasks = G``: the first G tasks are the iteration's train tasks (``loss_sum`` and the gradient cover them), the others its
    validation tasks (reference maml_vision.py:117-124), adapted and scored in the same launches without a backward half."""
    model = learner.module if isinstance(learner, MAML) else learner
    fo = learner.first_order if first_order is None and isinstance(learner, MAML) else bool(first_order)
    lr = learner.lr
    params = list(model.parameters())
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    spec = model.spec()
    if spec.ways != ways:
        raise ValueError(f'model has {spec.ways} outputs but ways={ways}')
    data = data.reshape(data.shape[0], data.shape[1], spec.in_channels, spec.in_h, spec.in_w).float().contiguous()
    ofs_flat = learner.offsets_flat() if isinstance(learner, MAML) else None
    if ofs_flat is not None:       # per-step offsets (StepOffsets): the offsets call, plain objective
        return _adapt_with_offsets(learner, model, data, labels, int(adaptation_steps), shots, fo, grad_tasks, None, ofs_flat)
    lr_flat = learner.lr_flat() if isinstance(learner, MAML) else None
    # step sizes per parameter (InnerLR, allow_nograd): the vector call, whose step sizes may want a gradient too
    need_lr = lr_flat is not None and torch.is_grad_enabled() and lr_flat.requires_grad
    return _FusedFastAdapt.apply(model.engine(), data, labels.contiguous(), shots, adaptation_steps, lr, fo, need or need_lr, need_lr, grad_tasks,
                                 lr_flat, *params)


def msl_weights(K, epoch, msl_epochs):
    """The per-step loss importance vector of MAML++ (Antoniou et al., 2019) for K inner steps: uniform 1/K at epoch 0, then the K - 1
    non-final weights decay linearly to the floor 0.03/K over ``msl_epochs`` epochs while the final one takes what they give up.
    Returns K floats that sum to 1 (w_1 .. w_K: the weight of the query loss after 1 .. K steps)."""
    K = int(K)
    if K < 1 or msl_epochs <= 0:
        raise ValueError('msl_weights needs K >= 1 and msl_epochs > 0')
    decay, floor = 1.0 / (K * msl_epochs), 0.03 / K
    w = [max(1.0 / K - epoch * decay, floor)] * (K - 1)
    return w + [min(1.0 / K + epoch * (K - 1) * decay, 1.0 - (K - 1) * floor)]


class _FusedFastAdaptSteps(torch.autograd.Function):
    """``_FusedFastAdapt`` through mi_meta_batch_maml_steps: the query loss and accuracy after every inner step, and the multi-step loss
    J = sum_t sum_j w_j L_query,t(theta_j) as the value that carries the gradients.  ``step_w`` [steps] lives on the device."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, steps, lr, first_order, need_grad, need_lr_grad, grad_tasks, step_w, lr_flat, *params):
        theta = flat_theta(params)
        lr_vec = None if lr_flat is None else lr_flat.detach().float().contiguous()
        if lr_vec is not None and lr_vec.shape[0] not in (1, max(int(steps), 1)):
            raise ValueError(f'the learner holds step sizes for {lr_vec.shape[0]} inner steps, the call adapts for {steps}')
        gt = data.shape[0] if grad_tasks is None else int(grad_tasks)

        def call(with_grad):
            return engine.meta_batch_steps(theta, data, labels, shots, steps, step_w, inner_lr=lr if lr_vec is None else None, lr_vec=lr_vec,
                                           first_order=first_order, grad_tasks=gt if with_grad else 0,
                                           want_lr_grad=with_grad and need_lr_grad and lr_vec is not None)[:4]
        ctx.deferred = call if need_grad and DEFERRED_OUTER_BACKWARD else None
        loss, acc, grad, lr_grad = call(need_grad and ctx.deferred is None)
        ctx.shapes = [p.shape for p in params]
        empty = torch.empty(0, device=data.device)
        ctx.save_for_backward(grad if grad is not None else empty, lr_grad if lr_grad is not None else empty)
        ctx.mark_non_differentiable(loss, acc)       # (values: only the objective carries the gradients, as in _FusedFastAdapt)
        return (step_w.unsqueeze(1) * loss[1:, :gt]).sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, lr_grad = ctx.saved_tensors
        if ctx.deferred is not None:
            _, _, grad, lr_grad = ctx.deferred(True)
            lr_grad = grad.new_empty(0) if lr_grad is None else lr_grad
        if grad.numel() == 0:
            raise RuntimeError('meta_batch_adapt_steps was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 11 + (lr_grad * gsum if lr_grad.numel() else None,) + split_grad(grad, ctx.shapes, gsum)


def meta_batch_adapt_steps(learner, data, labels, adaptation_steps, shots, ways, step_weights=None, first_order=None, grad_tasks=None):
    """``meta_batch_adapt`` with the query set scored after 0, 1, .., adaptation_steps inner steps in the one fused call, and the
    multi-step loss as the outer objective.  ``step_weights``: the K weights w_1 .. w_K of the query loss after 1 .. K steps (``msl_weights``;
    a list, or an fp32 tensor already on the device, which a caller may anneal in place); None: (0, .., 0, 1), the final loss only.
    Returns (objective, losses [K + 1, T], accs [K + 1, T]): objective = sum over the train tasks of sum_j w_j losses[j], and
    ``objective.backward()`` fills the base parameters' ``.grad`` (and a learnable ``InnerLR``'s) exactly as ``meta_batch_adapt`` does;
    under ``torch.no_grad()`` the call scores only.  losses and accs are plain values; row K is what ``meta_batch_adapt`` returns."""
    model = learner.module if isinstance(learner, MAML) else learner
    fo = learner.first_order if first_order is None and isinstance(learner, MAML) else bool(first_order)
    lr = learner.lr
    params = list(model.parameters())
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    spec = model.spec()
    if spec.ways != ways:
        raise ValueError(f'model has {spec.ways} outputs but ways={ways}')
    engine = model.engine()
    K = int(adaptation_steps)
    if step_weights is None:
        step_weights = [0.0] * (K - 1) + [1.0]
    if not torch.is_tensor(step_weights):
        step_weights = torch.tensor([float(w) for w in step_weights], dtype=torch.float32, device=data.device)
    data = data.reshape(data.shape[0], data.shape[1], spec.in_channels, spec.in_h, spec.in_w).float().contiguous()
    ofs_flat = learner.offsets_flat() if isinstance(learner, MAML) else None
    if ofs_flat is not None:       # per-step offsets (StepOffsets): the offsets call, multi-step loss
        return _adapt_with_offsets(learner, model, data, labels, K, shots, fo, grad_tasks, step_weights, ofs_flat)
    lr_flat = learner.lr_flat() if isinstance(learner, MAML) else None
    need_lr = lr_flat is not None and torch.is_grad_enabled() and lr_flat.requires_grad
    return _FusedFastAdaptSteps.apply(engine, data, labels.contiguous(), shots, K, lr, fo, need or need_lr, need_lr, grad_tasks,
                                      step_weights, lr_flat, *params)


def fast_adapt(batch, learner, loss, adaptation_steps, shots, ways, device, features=None):
    """Same signature/returns as the reference (vision.py:6-18): (valid_loss, valid_accuracy) as 0-dim tensors;
    ``valid_loss.backward()`` accumulates the (second-order unless learner.first_order) meta-gradient into the base
    module's parameters."""
    _check_loss(loss)
    data, labels = batch
    data, labels = data.to(device), labels.to(device)
    if features is not None:
        from .anil import fast_adapt_anil
        return fast_adapt_anil(data, labels, learner, features, adaptation_steps, shots, ways)
    total, losses, accs = meta_batch_adapt(learner, data.unsqueeze(0), labels.unsqueeze(0), adaptation_steps, shots, ways)
    return total, accs[0]


def accuracy(predictions, targets):
    """reference vision.py:21-23"""
    predictions = predictions.argmax(dim=1).view(targets.shape)
    return (predictions == targets).sum().float() / targets.size(0)


def evaluate(params, test_tasks, model, loss, device, features=None):
    """reference vision.py:26-42: mean query accuracy over params['meta_batch_size'] test tasks (no backward).  The tasks are
    sampled in the reference's order and then adapted in ONE batched engine call."""
    _check_loss(loss)
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        if features is None:
            data = torch.stack([b[0] for b in batches]).to(device)
            labels = torch.stack([b[1] for b in batches]).to(device)
            _, _, accs = meta_batch_adapt(model.clone(), data, labels, params['adapt_steps'], params['shots'], params['ways'])
            meta_test_accuracy = accs.mean().item()
        else:
            meta_test_accuracy = 0.0
            for b in batches:
                _, acc = fast_adapt(b, model.clone(), loss, params['adapt_steps'], params['shots'], params['ways'], device,
                                    features=features)
                meta_test_accuracy += acc.item()
            meta_test_accuracy /= params['meta_batch_size']
    print('Meta Test Accuracy', meta_test_accuracy)
    return meta_test_accuracy


def evaluate_steps(params, test_tasks, model, loss, device, features=None):
    """``evaluate`` per adaptation step: the mean query accuracy of params['meta_batch_size'] test tasks after 0, 1, ..,
    params['adapt_steps'] inner steps -- a list of adapt_steps + 1 floats, entry K being what ``evaluate`` returns -- from ONE fused
    call (the tasks are sampled in ``evaluate``'s order; the inner loop runs once, not once per step count).  ``features``: the ANIL
    trunk (``model`` is then the head's ``MAML``): one batched mi_meta_batch_anil_steps call."""
    _check_loss(loss)
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        data = torch.stack([b[0] for b in batches]).to(device)
        labels = torch.stack([b[1] for b in batches]).to(device)
        if features is None:
            _, _, accs = meta_batch_adapt_steps(model.clone(), data, labels, params['adapt_steps'], params['shots'], params['ways'])
        else:
            from .anil import meta_batch_adapt_anil_steps
            _, _, accs = meta_batch_adapt_anil_steps(model.clone(), features, data, labels, params['adapt_steps'], params['shots'], params['ways'])
        per_step = [a.item() for a in accs.mean(dim=1)]
    print('Meta Test Accuracy per step', per_step)
    return per_step
