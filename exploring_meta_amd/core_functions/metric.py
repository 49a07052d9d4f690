"""Metric heads on the 4-conv trunk: no inner loop at all.  The classifier is computed from the support features in closed form --
Prototypical Networks (``metric='proto'``: class means, logits = -scale * squared distance; learn2learn's ``protonet`` example) and NIL
(``metric='cosine'``: "No Inner Loop" of the ANIL paper, logits = scale * the summed cosine similarity to a class's support rows), both
through one fused HIP call (mi_meta_batch_metric: the ANIL call's trunk pass, one metric-head launch, the trunk backward).  ``features``
is what the ANIL entries take, and the engine is the ANIL one: a trunk trained with ``vision.anil_vision`` is scored here as it is."""
import torch

from ..engine import check_scale, metric_id
from .anil import _find_convbase, anil_engine
from .vision import flat_theta, split_grad
from .vision_models import MiniImagenetCNN, OmniglotCNN


class _FusedClosedForm(torch.autograd.Function):
    """``_FusedAnil`` with a closed-form head (``engine.meta_batch_<name>`` with the keyword arguments ``hyper``): the engine's theta carries
    zeros where its ANIL head sits.  ``params``: the logs of the first ``n_log`` values of ``hyper`` (the metric heads: none; the ridge
    head: log_lam, log_scale), then the trunk's parameters."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, name, hyper, n_log, need_grad, *params):
        trunk = flat_theta(params[n_log:])
        theta = torch.zeros(engine.param_count, dtype=torch.float32, device=trunk.device)
        theta[:trunk.numel()] = trunk
        loss, acc, grad, *dhyper = getattr(engine, f'meta_batch_{name}')(theta, data, labels, shots, with_grad=need_grad, **hyper)[:-1]
        ctx.shapes = [p.shape for p in params[n_log:]]
        ctx.name, ctx.hyper = name, tuple(hyper.values())[:n_log]
        none = torch.empty(0, device=data.device)
        # the hyper-parameters' gradient: the sum of the per-task rows (one reduction of ours, in a fixed order)
        ctx.save_for_backward(grad[:trunk.numel()] if grad is not None else none,
                              dhyper[0].double().sum(dim=0) if dhyper and grad is not None else none)
        # Only the SUM carries the meta-gradient (the engine reduces over tasks inside the fused call): the per-task losses are
        # values, so `losses.mean().backward()` fails loudly instead of stepping on zeros.
        ctx.mark_non_differentiable(loss, acc)
        return loss.sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        grad, dh = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError(f'meta_batch_adapt_{ctx.name} was run without gradients (torch.no_grad or no parameter requires grad)')
        # d/dlog(x) = x d/dx
        dlog = tuple((dh[i] * x).float() * gsum if ctx.needs_input_grad[8 + i] else None for i, x in enumerate(ctx.hyper))
        return (None,) * 8 + dlog + split_grad(grad, ctx.shapes, gsum)


def _trunk_of(features):
    """The ConvBase of a ``ConvBase``, an ANIL ``features`` Sequential or a ``MiniImagenetCNN``; a mean-pooled ``OmniglotCNN`` has none
    whose flattened output is what its head saw."""
    if isinstance(features, OmniglotCNN):
        raise NotImplementedError('OmniglotCNN feeds its head the spatial MEAN of the trunk output; the metric heads score the flattened '
                                  'feature vector (use an ANIL trunk: vision.anil_vision / vision.protonet_vision)')
    if isinstance(features, MiniImagenetCNN):
        return features.base
    return _find_convbase(features)


def _closed_form_adapt(name, features, data, labels, shots, ways, hyper, log_hyper=()):
    """One fused call of the closed-form head ``name`` on the trunk of ``features``: ``hyper`` its checked keyword arguments, ``log_hyper``
    the tensors that hold the logs of the first of them (a gradient for each that requires one)."""
    base = _trunk_of(features)
    engine = anil_engine(base, ways, data.shape[-2], data.device)
    params = list(base.parameters())
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params + list(log_hyper))
    log_hyper = tuple(h.to(data.device) for h in log_hyper)
    return _FusedClosedForm.apply(engine, data.float().contiguous(), labels.contiguous(), shots, name, hyper, len(log_hyper), need,
                                  *log_hyper, *params)


def _fast_adapt(batch, device, adapt):
    """One task through a batched entry ``adapt(data [1, ...], labels [1, ...])``, with ``fast_adapt``'s returns."""
    data, labels = batch
    total, _, accs = adapt(data.to(device).unsqueeze(0), labels.to(device).unsqueeze(0))
    return total, accs[0]


def _score_test_tasks(params, test_tasks, features, device, adapt):
    """The mean query accuracy of params['meta_batch_size'] test tasks, sampled in ``evaluate``'s order, from ONE batched call
    ``adapt(base, data, labels)`` without a gradient.  The caller has refused what it refuses: no task is drawn before that."""
    base = _trunk_of(features)
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        data = torch.stack([b[0] for b in batches]).to(device)
        labels = torch.stack([b[1] for b in batches]).to(device)
        data = data.reshape(data.shape[0], data.shape[1], base.channels, *data.shape[-2:])
        _, _, accs = adapt(base, data, labels)
        return accs.mean().item()


def meta_batch_adapt_metric(features, data, labels, shots, ways, metric='proto', scale=1.0):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU -> (loss_sum, loss[T], acc[T]).  ``loss_sum.backward()``
    fills ``.grad`` of the trunk's parameters and of nothing else; under ``torch.no_grad()`` the call only scores.  loss and acc are
    plain values, as in ``meta_batch_adapt_anil``."""
    metric_id(metric)
    return _closed_form_adapt('metric', features, data, labels, shots, ways, dict(metric=metric, scale=check_scale(scale)))


def fast_adapt_metric(batch, features, shots, ways, device, metric='proto', scale=1.0):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    return _fast_adapt(batch, device, lambda d, l: meta_batch_adapt_metric(features, d, l, shots, ways, metric=metric, scale=scale))


def evaluate_nil(params, test_tasks, features, device, metric='cosine', scale=1.0):
    """The counterpart of ``evaluate`` without an inner loop: the mean query accuracy of params['meta_batch_size'] test tasks, sampled in
    ``evaluate``'s order, from ONE batched call without a gradient.  ``features``: a ``ConvBase``, an ANIL ``features`` Sequential or a
    ``MiniImagenetCNN`` (its ``.base``; the head is thrown away).  How good are the features alone?"""
    metric_id(metric)
    scale = check_scale(scale)
    nil_test_accuracy = _score_test_tasks(params, test_tasks, features, device, lambda base, d, l: meta_batch_adapt_metric(
        base, d, l, params['shots'], params['ways'], metric=metric, scale=scale))
    print('NIL Test Accuracy', nil_test_accuracy)
    return nil_test_accuracy
