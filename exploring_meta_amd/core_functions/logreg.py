"""The logistic-regression head on the 4-conv trunk: the head's own inner problem under the loss ANIL's inner loop runs -- softmax
cross-entropy with an L2 regulariser -- solved to optimality on the support set and differentiated through the optimum by the implicit
function theorem, not through K unrolled steps (LR-D2 of the R2-D2 paper for any number of classes; the convex head of MetaOptNet; the
test-time classifier of "Rethinking Few-Shot Image Classification").  One fused HIP call (mi_meta_batch_logreg: the ANIL call's trunk
pass, one head launch that solves every task by Newton + conjugate gradients in fp64 and differentiates through the solution, the trunk
backward).  Per task, with the support / query features fs / fq:

    W* = argmin_W  sum_i CE(W fs_i, ys_i) + lam/2 |W|^2        logits = scale * fq W*^T

``lam`` (the regulariser) and ``scale`` (the logit scale) are the head's two hyper-parameters, meta-learned by default (``LogRegHead``).
There is no bias.  ``features`` is what the ANIL entries take, and the engine is the ANIL one: a trunk trained with
``vision.anil_vision`` is scored here as it is -- "does truncating the head's loop at K steps matter, or only the features?"."""
from ..engine import check_logreg
from .metric import _closed_form_adapt, _fast_adapt, _score_test_tasks
from .ridge import RidgeHead


class LogRegHead(RidgeHead):
    """The head's two scalars, held as ``log_lam`` and ``log_scale`` exactly as ``RidgeHead`` holds its own (positivity without clamping,
    the chain rule in metric._FusedClosedForm, learnable=False: buffers): the same storage under this head's own name and checks."""

    def __init__(self, lam=1.0, scale=1.0, learnable=True):
        lam, scale = check_logreg(lam, scale)
        super().__init__(lam, scale, learnable)


def _check_head(head):
    if not isinstance(head, LogRegHead):
        raise TypeError(f'head must be a LogRegHead, got {type(head).__name__}')
    return check_logreg(head.lam, head.scale)


def meta_batch_adapt_logreg(features, head, data, labels, shots, ways):
    """Batched entry: data [T, 2*S*W, C, H, W], labels [T, 2*S*W] on the GPU, head a ``LogRegHead`` -> (loss_sum, loss[T], acc[T]).
    ``loss_sum.backward()`` fills ``.grad`` of the trunk's parameters and of the head's two (the sum of the per-task rows); under
    ``torch.no_grad()`` the call only scores.  loss and acc are plain values, as in ``meta_batch_adapt_metric``."""
    lam, scale = _check_head(head)
    return _closed_form_adapt('logreg', features, data, labels, shots, ways, dict(lam=lam, scale=scale), (head.log_lam, head.log_scale))


def fast_adapt_logreg(batch, features, head, shots, ways, device):
    """The one-task form, with ``fast_adapt``'s returns: (valid_loss, valid_accuracy) as 0-dim tensors."""
    return _fast_adapt(batch, device, lambda d, l: meta_batch_adapt_logreg(features, head, d, l, shots, ways))


def evaluate_logreg(params, test_tasks, features, head, device):
    """The counterpart of ``evaluate`` with the head solved to convergence: the mean query accuracy of params['meta_batch_size'] test
    tasks, sampled in ``evaluate``'s order, from ONE batched call without a gradient.  ``features`` as for ``evaluate_nil``."""
    _check_head(head)
    logreg_test_accuracy = _score_test_tasks(params, test_tasks, features, device, lambda base, d, l: meta_batch_adapt_logreg(
        base, head, d, l, params['shots'], params['ways']))
    print('LogReg Test Accuracy', logreg_test_accuracy)
    return logreg_test_accuracy
