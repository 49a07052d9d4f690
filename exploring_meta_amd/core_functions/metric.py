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


class _FusedMetric(torch.autograd.Function):
    """``_FusedAnil`` without a head: ``params`` are the trunk's; the engine's theta carries zeros where its ANIL head sits."""

    @staticmethod
    def forward(ctx, engine, data, labels, shots, metric, scale, need_grad, *params):
        trunk = flat_theta(params)
        theta = torch.zeros(engine.param_count, dtype=torch.float32, device=trunk.device)
        theta[:trunk.numel()] = trunk
        loss, acc, grad, _ = engine.meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale, with_grad=need_grad)
        ctx.shapes = [p.shape for p in params]
        ctx.save_for_backward(grad[:trunk.numel()] if grad is not None else torch.empty(0, device=data.device))
        # Only the SUM carries the meta-gradient (the engine reduces over tasks inside the fused call): the per-task losses are
        # values, so `losses.mean().backward()` fails loudly instead of stepping on zeros.
        ctx.mark_non_differentiable(loss, acc)
        return loss.sum(), loss, acc

    @staticmethod
    def backward(ctx, gsum, gloss, gacc):
        (grad,) = ctx.saved_tensors
        if grad.numel() == 0:
            raise RuntimeError('meta_batch_adapt_metric was run without gradients (torch.no_grad or no parameter requires grad)')
        return (None,) * 7 + split_grad(grad, ctx.shapes, gsum)


def _trunk_of(features):
    """The ConvBase of a ``ConvBase``, an ANIL ``features`` Sequential or a ``MiniImagenetCNN``; a mean-pooled ``OmniglotCNN`` has none
    whose flattened output is what its head saw."""
    if isinstance(features, OmniglotCNN):
        raise NotImplementedError('OmniglotCNN feeds its head the spatial MEAN of the trunk output; the metric heads score the flattened '
                                  'feature vector (use an ANIL trunk: vision.anil_vision / vision.protonet_vision)')
    if isinstance(features, MiniImagenetCNN):
        return features.base
    return _find_convbase(features)


def meta_batch_adapt_metric(features, data, labels, shots, ways, metric='proto', scale=1.0):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU -> (loss_sum, loss[T], acc[T]).  ``loss_sum.backward()``
    fills ``.grad`` of the trunk's parameters and of nothing else; under ``torch.no_grad()`` the call only scores.  loss and acc are
    plain values, as in ``meta_batch_adapt_anil``."""
    metric_id(metric)
    scale = check_scale(scale)
    base = _trunk_of(features)
    engine = anil_engine(base, ways, data.shape[-2], data.device)
    params = list(base.parameters())
    need = torch.is_grad_enabled() and any(p.requires_grad for p in params)
    return _FusedMetric.apply(engine, data.float().contiguous(), labels.contiguous(), shots, metric, scale, need, *params)


def fast_adapt_metric(batch, features, shots, ways, device, metric='proto', scale=1.0):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    data, labels = batch
    total, _, accs = meta_batch_adapt_metric(features, data.to(device).unsqueeze(0), labels.to(device).unsqueeze(0), shots, ways,
                                             metric=metric, scale=scale)
    return total, accs[0]


def evaluate_nil(params, test_tasks, features, device, metric='cosine', scale=1.0):
    """The counterpart of ``evaluate`` without an inner loop: the mean query accuracy of params['meta_batch_size'] test tasks, sampled in
    ``evaluate``'s order, from ONE batched call without a gradient.  ``features``: a ``ConvBase``, an ANIL ``features`` Sequential or a
    ``MiniImagenetCNN`` (its ``.base``; the head is thrown away).  How good are the features alone?"""
    metric_id(metric)
    scale = check_scale(scale)
    base = _trunk_of(features)
    batches = [test_tasks.sample() for _ in range(params['meta_batch_size'])]
    with torch.no_grad():
        data = torch.stack([b[0] for b in batches]).to(device)
        labels = torch.stack([b[1] for b in batches]).to(device)
        data = data.reshape(data.shape[0], data.shape[1], base.channels, *data.shape[-2:])
        _, _, accs = meta_batch_adapt_metric(base, data, labels, params['shots'], params['ways'], metric=metric, scale=scale)
        nil_test_accuracy = accs.mean().item()
    print('NIL Test Accuracy', nil_test_accuracy)
    return nil_test_accuracy
