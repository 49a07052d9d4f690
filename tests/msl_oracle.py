"""Oracle (TEST INFRASTRUCTURE) for the multi-step loss and the per-step query metrics of the fused MAML call
(mi_meta_batch_maml_steps): the autograd restatement of oracle/vision_ref.py (prepare_batch, model_forward, clone_params) whose outer
objective is sum_j w_j CE(query at theta_j), j = 1..K, with a scalar inner step or the per-parameter step sizes of
tests/inner_lr_oracle.py as leaves.  It scores the query set at every theta_j, j = 0..K (loss, accuracy, logits).  Plus the closed form
the engine implements, for the host test that pins one against the other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vision_ref as R
from inner_lr_oracle import lr_vector, lr_dict, _row  # noqa: F401  (lr_vector: re-exported for the tests' step sizes)


def _is_scalar(lr):
    return np.ndim(lr) == 0


def meta_batch(theta, spec, datas, labelss, K, shots, ways, lr, step_w, first_order, dtype=torch.float64, grad_tasks=None):
    """lr: a number (the scalar step) or a flat [steps, P] array (steps 1 or K).  step_w: K weights w_1..w_K.  The first grad_tasks tasks
    (None: all) carry the objective.  Returns a dict of numpy arrays: losses [K + 1, T], accs [K + 1, T], logits [K + 1, T, n, ways],
    meta_grad [P], lr_grad [steps, P] (None for a scalar step)."""
    so = not first_order
    T = len(datas)
    gt = T if grad_tasks is None else grad_tasks
    w = [float(x) for x in np.asarray(step_w, dtype=np.float64)]
    assert len(w) == K >= 1
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta.items())
    lrs = None if _is_scalar(lr) else lr_dict(spec, lr, dtype)
    losses, accs, logits = np.zeros((K + 1, T)), np.zeros((K + 1, T)), [[None] * T for _ in range(K + 1)]
    for t, (data, labels) in enumerate(zip(datas, labelss)):
        p = R.clone_params(leaves)
        ad, al, ed, el = R.prepare_batch(data.to(dtype), labels, shots, ways)
        objective = 0.0
        for j in range(K + 1):
            pred = R.model_forward(ed, p, spec)
            lq = F.cross_entropy(pred, el)
            losses[j, t], accs[j, t], logits[j][t] = float(lq.detach()), float(R.accuracy(pred, el)), pred.detach().double().numpy()
            if j >= 1 and t < gt:
                objective = objective + w[j - 1] * lq
            if j == K:
                break
            loss = F.cross_entropy(R.model_forward(ad, p, spec), al)
            gs = torch.autograd.grad(loss, list(p.values()), retain_graph=so, create_graph=so)
            step = (lambda n: float(lr)) if lrs is None else (lambda n: _row(lrs, n, j))
            p = OrderedDict((n, v - step(n) * g) for (n, v), g in zip(p.items(), gs))
        if t < gt:
            objective.backward()
    g = R.flatten_params(OrderedDict((k, v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in leaves.items()))
    lg = None
    if lrs is not None:
        steps = next(iter(lrs.values())).shape[0]
        lg = torch.cat([(v.grad if v.grad is not None else torch.zeros_like(v)).reshape(steps, -1) for v in lrs.values()], dim=1).double().numpy()
    return dict(losses=losses, accs=accs, logits=np.asarray(logits), meta_grad=g.detach().double().numpy(), lr_grad=lg)


def closed_form(theta, spec, datas, labelss, K, shots, ways, lr, step_w, first_order, dtype=torch.float64):
    """What the engine computes.  q_j = grad L_query(theta_j); second order lam_K = w_K q_K, lam_k = lam_{k+1} - H_k (D_k lam_{k+1}) + w_k q_k
    (k = K-1..1), lam_0 = lam_1 - H_0 (D_0 lam_1); first order lam_k = sum_{j >= max(k, 1)} w_j q_j; meta_grad = sum_t lam_0,
    lr_grad_k = -sum_t g_k * lam_{k+1}.  Every Hessian-vector product by double backward.  Returns (meta_grad [P], lr_grad [steps, P] or None)."""
    names = list(theta.keys())
    w = [float(x) for x in np.asarray(step_w, dtype=np.float64)]
    lrs = None if _is_scalar(lr) else lr_dict(spec, lr, dtype)
    steps = 1 if lrs is None else next(iter(lrs.values())).shape[0]
    step = (lambda n, k: float(lr)) if lrs is None else (lambda n, k: _row(lrs, n, k).detach())
    P = sum(v.numel() for v in theta.values())
    meta, lrg = torch.zeros(P, dtype=dtype), torch.zeros(steps, P, dtype=dtype)
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    for data, labels in zip(datas, labelss):
        ad, al, ed, el = R.prepare_batch(data.to(dtype), labels, shots, ways)
        th = [OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta.items())]
        gs = []
        for k in range(K):
            loss = F.cross_entropy(R.model_forward(ad, th[k], spec), al)
            g = torch.autograd.grad(loss, list(th[k].values()), create_graph=True)
            gs.append(g)
            th.append(OrderedDict((n, (v - step(n, k) * gi).detach().requires_grad_(True)) for (n, v), gi in zip(th[k].items(), g)))
        q = [None] + [[x.detach() for x in torch.autograd.grad(F.cross_entropy(R.model_forward(ed, th[j], spec), el), list(th[j].values()))]
                      for j in range(1, K + 1)]
        lam = [w[K - 1] * x for x in q[K]]                                         # lam_K
        for k in range(K - 1, -1, -1):                                            # lam holds lam_{k+1}
            lrg[k if steps > 1 else 0] -= flat([gi.detach() * li for gi, li in zip(gs[k], lam)])
            if not first_order:
                d = [step(n, k) * li for n, li in zip(names, lam)]
                hv = torch.autograd.grad(gs[k], list(th[k].values()), grad_outputs=d, allow_unused=True)
                lam = [li - (h if h is not None else torch.zeros_like(li)) for li, h in zip(lam, hv)]
            if k >= 1:
                lam = [li + w[k - 1] * qi for li, qi in zip(lam, q[k])]
        meta += flat(lam)
    return meta.double().numpy(), (None if lrs is None else lrg.double().numpy())
