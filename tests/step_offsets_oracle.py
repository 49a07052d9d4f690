"""Oracle (TEST INFRASTRUCTURE) for per-step parameter offsets in the fused MAML call (mi_meta_batch_maml_offsets): tests/msl_oracle.py's
autograd restatement with the update ``p <- v - step * g + s_{j+1}`` and the offsets as autograd leaves, so that autograd gives the
gradient of the objective with respect to them.  Plus the closed form the engine implements -- the unchanged adjoint recursion on the
shifted trajectory, offsets_grad[k] = sum_t lam_{k+1} -- for the host test that pins one against the other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vision_ref as R
from inner_lr_oracle import lr_vector, lr_dict, _row  # noqa: F401  (lr_vector: re-exported for the tests' step sizes)


def _is_scalar(lr):
    return np.ndim(lr) == 0


def offsets_array(spec, K, seed, std=0.05, tensors='bn+bias'):
    """[K, P] fp32 offsets in parameters() order, N(0, std^2) (a pure function of the seed) on the selected tensors and zero elsewhere:
    'bn+bias' = the BatchNorm tensors and linear.bias (the standard offsets), 'bn' = the BatchNorm tensors, 'all' = every tensor."""
    shapes = R.param_shapes(spec)
    P = sum(int(np.prod(s)) for s in shapes.values())
    v = (std * np.random.RandomState(seed).standard_normal((K, P))).astype(np.float32)
    off = 0
    for name, shp in shapes.items():
        n = int(np.prod(shp))
        keep = tensors == 'all' or '.normalize.' in name or (tensors == 'bn+bias' and name == 'linear.bias')
        if not keep:
            v[:, off:off + n] = 0.0
        off += n
    return v


def final_only(K):
    return [0.0] * (K - 1) + [1.0]


def meta_batch(theta, spec, datas, labelss, K, shots, ways, lr, step_w, offsets, first_order, dtype=torch.float64, grad_tasks=None):
    """tests/msl_oracle.py::meta_batch with offsets [K, P] (row j is added after inner step j).  step_w None: the plain objective
    (w = (0, .., 0, 1)).  Returns its dict plus offsets_grad [K, P]."""
    so = not first_order
    T = len(datas)
    gt = T if grad_tasks is None else grad_tasks
    w = [float(x) for x in np.asarray(final_only(K) if step_w is None else step_w, dtype=np.float64)]
    assert len(w) == K >= 1 and np.shape(offsets)[0] == K
    leaves = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta.items())
    lrs = None if _is_scalar(lr) else lr_dict(spec, lr, dtype)
    ofs = lr_dict(spec, offsets, dtype)            # name -> [K, *shape] leaves
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
            p = OrderedDict((n, v - step(n) * g + ofs[n][j]) for (n, v), g in zip(p.items(), gs))
        if t < gt:
            objective.backward()
    zg = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
    g = R.flatten_params(OrderedDict((k, zg(v)) for k, v in leaves.items()))
    lg = None
    if lrs is not None:
        steps = next(iter(lrs.values())).shape[0]
        lg = torch.cat([zg(v).reshape(steps, -1) for v in lrs.values()], dim=1).double().numpy()
    og = torch.cat([zg(v).reshape(K, -1) for v in ofs.values()], dim=1).double().numpy()
    return dict(losses=losses, accs=accs, logits=np.asarray(logits), meta_grad=g.detach().double().numpy(), lr_grad=lg, offsets_grad=og)


def closed_form(theta, spec, datas, labelss, K, shots, ways, lr, step_w, offsets, first_order, dtype=torch.float64):
    """What the engine computes: tests/msl_oracle.py::closed_form on the trajectory theta_{k+1} = (theta_k - D_k g_k) + s_{k+1}, and
    offsets_grad[k] = sum_t lam_{k+1} (lam_{k+1} complete: its w_{k+1} q_{k+1} in).  Returns (meta_grad [P], lr_grad [steps, P] or None,
    offsets_grad [K, P])."""
    names = list(theta.keys())
    w = [float(x) for x in np.asarray(final_only(K) if step_w is None else step_w, dtype=np.float64)]
    lrs = None if _is_scalar(lr) else lr_dict(spec, lr, dtype)
    ofs = lr_dict(spec, offsets, dtype)
    steps = 1 if lrs is None else next(iter(lrs.values())).shape[0]
    step = (lambda n, k: float(lr)) if lrs is None else (lambda n, k: _row(lrs, n, k).detach())
    P = sum(v.numel() for v in theta.values())
    meta, lrg, og = torch.zeros(P, dtype=dtype), torch.zeros(steps, P, dtype=dtype), torch.zeros(K, P, dtype=dtype)
    flat = lambda ts: torch.cat([t.reshape(-1) for t in ts])
    for data, labels in zip(datas, labelss):
        ad, al, ed, el = R.prepare_batch(data.to(dtype), labels, shots, ways)
        th = [OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta.items())]
        gs = []
        for k in range(K):
            loss = F.cross_entropy(R.model_forward(ad, th[k], spec), al)
            g = torch.autograd.grad(loss, list(th[k].values()), create_graph=True)
            gs.append(g)
            th.append(OrderedDict((n, (v - step(n, k) * gi + ofs[n][k]).detach().requires_grad_(True)) for (n, v), gi in zip(th[k].items(), g)))
        q = [None] + [[x.detach() for x in torch.autograd.grad(F.cross_entropy(R.model_forward(ed, th[j], spec), el), list(th[j].values()))]
                      for j in range(1, K + 1)]
        lam = [w[K - 1] * x for x in q[K]]                                         # lam_K
        for k in range(K - 1, -1, -1):                                            # lam holds lam_{k+1}
            og[k] += flat(lam)
            lrg[k if steps > 1 else 0] -= flat([gi.detach() * li for gi, li in zip(gs[k], lam)])
            if not first_order:
                d = [step(n, k) * li for n, li in zip(names, lam)]
                hv = torch.autograd.grad(gs[k], list(th[k].values()), grad_outputs=d, allow_unused=True)
                lam = [li - (h if h is not None else torch.zeros_like(li)) for li, h in zip(lam, hv)]
            if k >= 1:
                lam = [li + w[k - 1] * qi for li, qi in zip(lam, q[k])]
        meta += flat(lam)
    return meta.double().numpy(), (None if lrs is None else lrg.double().numpy()), og.double().numpy()
