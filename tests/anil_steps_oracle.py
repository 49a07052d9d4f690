"""Oracle (TEST INFRASTRUCTURE) for the vector-step and multi-step-loss ANIL calls (mi_meta_batch_anil_lr, mi_meta_batch_anil_steps;
DESIGN.md section 23): the autograd restatement of the reference's ANIL train half on oracle/vision_ref.py (conv_base, head_forward,
prepare_batch, clone_params) whose head update is ``v - lr[name][step] * g`` with the step sizes as leaves [steps, Ph], and whose outer
objective is sum_j w_j CE(query at theta_j), j = 1..K.  It scores the query set at every theta_j, j = 0..K.  Plus the closed form the
engine implements, for the host test that pins one against the other, and the fixtures both test files share."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from helpers import hash_params, task_tensors

HEAD = ('weight', 'bias')

# name: dataset of the synthetic tasks, trunk (hidden, channels, max_pool), input side, fc_neurons, ways, shots
SHAPES = {
    'omni': ('omni', (32, 1, False), 28, 128, 5, 1),       # Omniglot ANIL 5-way 1-shot: hidden 32, stride 2, Ph = 645
    'omni3w2s': ('omni', (32, 1, False), 28, 128, 3, 2),   # Ph = 387
    'min': ('min', (64, 3, True), 84, 1600, 5, 5),         # Mini-ImageNet ANIL 5-way 5-shot: the 5x5 column permutation, Ph = 8005
}


# the synthetic task ids of the GPU test (tests/test_gpu_anil_steps.py); tests/test_anil_steps_host.py asserts that the fp64 oracle leaves
# at most one row in ten of any (step, task) under the accuracy margin on them
GPU_TASKS = {'omni': [0, 1, 2], 'omni3w2s': [0, 1], 'min': [0, 1]}


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def fixtures(shape, dtype=torch.float64):
    """(base spec, trunk parameters, head parameters, fc_neurons, ways, shots) of a shape: the parameters of tests/test_gpu_anil.py."""
    _, (hidden, channels, max_pool), hw, fc, ways, shots = SHAPES[shape]
    base = R.convbase_spec(hidden, channels, max_pool)
    spec = dict(kind='min', in_shape=(channels, hw, hw), base=base)
    tf = hash_params(R.param_shapes(spec, prefix_base='0.'), 13, dtype)
    th = hash_params({'weight': (ways, fc), 'bias': (ways,)}, 17, dtype)
    return base, tf, th, fc, ways, shots


def tasks(shape, task_ids, dtype=torch.float64):
    """The synthetic tasks as the oracle takes them: lists of [2n, C, H, W] data and [2n] labels."""
    dataset, (_, channels, _), hw, _, ways, shots = SHAPES[shape]
    datas, labels = task_tensors(dataset, task_ids, ways, shots, dtype)
    return [d.view(-1, channels, hw, hw) for d in datas], labels


def head_count(fc, ways):
    return ways * fc + ways


def lr_vector(fc, ways, base, steps, seed, frozen=()):
    """[steps, Ph] fp32 step sizes in head.parameters() order (weight, bias): base * U(0.5, 1.5) per entry, a pure function of the seed;
    0 on the tensors named in ``frozen``."""
    v = (base * (0.5 + synthetic.hash_uniform(seed, (steps, head_count(fc, ways))))).astype(np.float32)
    if 'weight' in frozen:
        v[:, :ways * fc] = 0.0
    if 'bias' in frozen:
        v[:, ways * fc:] = 0.0
    return v


def _is_scalar(lr):
    return np.ndim(lr) == 0


def _lr_leaves(lr, fc, ways, dtype):
    flat = torch.as_tensor(np.asarray(lr)).to(dtype).reshape(-1, head_count(fc, ways))
    return OrderedDict((('weight', flat[:, :ways * fc].reshape(-1, ways, fc).clone().requires_grad_(True)),
                        ('bias', flat[:, ways * fc:].clone().requires_grad_(True))))


def _row(lrs, name, k):
    t = lrs[name]
    return t[k if t.shape[0] > 1 else 0]


def _flat(ts):
    return torch.cat([t.reshape(-1) for t in ts])


def meta_batch(theta_feat, theta_head, base, fc, datas, labelss, K, shots, ways, lr, step_w, first_order, dtype=torch.float64):
    """lr: a number (the scalar step) or a flat [steps, Ph] array (steps 1 or K).  step_w: K weights w_1..w_K (K = 0: none; the loss at
    theta_0 is then the objective, as in the plain call).  Returns a dict of numpy arrays: losses [K + 1, T], accs [K + 1, T], logits
    [K + 1, T, n, ways], grad_feat, grad_head (flat, parameters() order), lr_grad [steps, Ph] (None for a scalar step)."""
    so = not first_order
    T = len(datas)
    w = [float(x) for x in np.asarray(step_w, dtype=np.float64)]
    assert len(w) == K
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    hl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_head.items())
    lrs = None if _is_scalar(lr) else _lr_leaves(lr, fc, ways, dtype)
    feats = lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc)
    losses, accs, logits = np.zeros((K + 1, T)), np.zeros((K + 1, T)), [[None] * T for _ in range(K + 1)]
    for t, (data, labels) in enumerate(zip(datas, labelss)):
        p = R.clone_params(hl)
        ad, al, ed, el = R.prepare_batch(data.to(dtype), labels, shots, ways, feats)
        objective = 0.0
        for j in range(K + 1):
            pred = R.head_forward(ed, p)
            lq = F.cross_entropy(pred, el)
            losses[j, t], accs[j, t], logits[j][t] = float(lq.detach()), float(R.accuracy(pred, el)), pred.detach().double().numpy()
            if j >= 1:
                objective = objective + w[j - 1] * lq
            if j == K:
                break
            loss = F.cross_entropy(R.head_forward(ad, p), al)
            gs = torch.autograd.grad(loss, list(p.values()), retain_graph=True, create_graph=so)
            step = (lambda n: float(lr)) if lrs is None else (lambda n: _row(lrs, n, j))
            p = OrderedDict((n, v - step(n) * g) for (n, v), g in zip(p.items(), gs))
        (objective if K >= 1 else lq).backward()
    zero = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
    lg = None
    if lrs is not None:
        steps = lrs['weight'].shape[0]
        lg = torch.cat([zero(lrs[n]).reshape(steps, -1) for n in HEAD], dim=1).double().numpy()
    return dict(losses=losses, accs=accs, logits=np.asarray(logits), grad_feat=_flat([zero(v) for v in fl.values()]).double().numpy(),
                grad_head=_flat([zero(v) for v in hl.values()]).double().numpy(), lr_grad=lg)


def closed_form(theta_feat, theta_head, base, fc, datas, labelss, K, shots, ways, lr, step_w, first_order, dtype=torch.float64):
    """What the engine computes (K >= 1), per task with the features f_s, f_q of ONE trunk pass:
      q_j = grad_theta L_q(theta_j), dq_j = dL_q(theta_j)/df_q;  df_q = sum_j w_j dq_j
      second order: lam_K = w_K q_K, lam_k = lam_{k+1} - H_k (D_k lam_{k+1}) + w_k q_k, lam_0 = lam_1 - H_0 (D_0 lam_1),
                    df_s = -sum_k R_{D_k lam_{k+1}}{dL_s/df_s}(theta_k)  (= -d/df_s <g_k, dir>, dir held constant)
      first order:  lam_k = sum_{j >= max(k, 1)} w_j q_j, df_s = 0
      head gradient = sum_t lam_0; trunk gradient = one backward of the features from [df_s, df_q]; lr_grad_k = -sum_t g_k * lam_{k+1}.
    Returns (grad_feat, grad_head, lr_grad [steps, Ph] or None) as numpy."""
    w = [float(x) for x in np.asarray(step_w, dtype=np.float64)]
    assert len(w) == K >= 1
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    lrs = None if _is_scalar(lr) else OrderedDict((n, v.detach()) for n, v in _lr_leaves(lr, fc, ways, dtype).items())
    steps = 1 if lrs is None else lrs['weight'].shape[0]
    step = (lambda n, k: float(lr)) if lrs is None else (lambda n, k: _row(lrs, n, k))
    Ph = head_count(fc, ways)
    head, lrg = torch.zeros(Ph, dtype=dtype), torch.zeros(steps, Ph, dtype=dtype)
    for data, labels in zip(datas, labelss):
        f = R.conv_base(data.to(dtype), fl, base, prefix='0.').view(-1, fc)
        fs_, al, fq_, el = R.prepare_batch(f, labels, shots, ways)
        fs, fq = fs_.detach().requires_grad_(True), fq_.detach().requires_grad_(True)
        th = [OrderedDict((n, theta_head[n].detach().to(dtype).clone().requires_grad_(True)) for n in HEAD)]
        gs = []
        for k in range(K):
            g = torch.autograd.grad(F.cross_entropy(R.head_forward(fs, th[k]), al), list(th[k].values()), create_graph=True)
            gs.append(g)
            th.append(OrderedDict((n, (v - step(n, k) * gi).detach().requires_grad_(True)) for (n, v), gi in zip(th[k].items(), g)))
        q, dfq = [None], torch.zeros_like(fq)
        for j in range(1, K + 1):
            out = torch.autograd.grad(F.cross_entropy(R.head_forward(fq, th[j]), el), list(th[j].values()) + [fq])
            q.append([x.detach() for x in out[:2]])
            dfq = dfq + w[j - 1] * out[2].detach()
        lam = [w[K - 1] * x for x in q[K]]
        dfs = torch.zeros_like(fs)
        for k in range(K - 1, -1, -1):                     # lam holds lam_{k+1}
            lrg[k if steps > 1 else 0] -= _flat([gi.detach() * li for gi, li in zip(gs[k], lam)])
            if not first_order:
                d = [step(n, k) * li for n, li in zip(HEAD, lam)]
                out = torch.autograd.grad(gs[k], list(th[k].values()) + [fs], grad_outputs=d, retain_graph=True)
                lam = [li - h for li, h in zip(lam, out[:2])]
                dfs = dfs - out[2]
            if k >= 1:
                lam = [li + w[k - 1] * qi for li, qi in zip(lam, q[k])]
        head += _flat(lam)
        torch.autograd.backward([fs_, fq_], [dfs, dfq])
    gf = _flat([v.grad if v.grad is not None else torch.zeros_like(v) for v in fl.values()])
    return gf.double().numpy(), head.double().numpy(), (None if lrs is None else lrg.double().numpy())


def clear_rows(logits64):
    """[K + 1, T, n] bool: the rows whose fp64 top-2 logit margin exceeds 1e-3 * max(1, |logits| of that (step, task))."""
    top2 = np.sort(logits64, axis=-1)[..., -2:]
    scale = np.maximum(1.0, np.abs(logits64).max(axis=(-2, -1)))[..., None]
    return (top2[..., 1] - top2[..., 0]) > 1e-3 * scale


# The cases tests/test_gpu_anil_steps.py holds to this oracle (tests/test_anil_steps_host.py asserts the margin property on each of them).
BASE_LR = 0.4
ORACLE_CASES = {
    # (task 0 with a frozen bias leaves one of its five rows under the accuracy margin at step 2 in fp64: those cases take tasks 1..3)
    # name: shape, task ids, K, entry ('steps' / 'lr'), step ('scalar' / 'vector' / 'per_step' / 'frozen_bias'), first order, weights,
    #       gradient floor (the bars of tests/test_gpu_anil.py for the same trunk)
    'omni_steps_so_per_step': ('omni', (0, 1, 2), 2, 'steps', 'per_step', False, (0.3, 0.7), 1e-3),
    'omni_steps_so_scalar_K3': ('omni', (0, 1, 2), 3, 'steps', 'scalar', False, (0.2, 0.3, 0.5), 1e-3),
    'omni_steps_fo_frozen_bias_K3': ('omni', (1, 2, 3), 3, 'steps', 'frozen_bias', True, (0.2, 0.3, 0.5), 1e-3),
    'omni_steps_so_vector_K3': ('omni', (0, 1, 2), 3, 'steps', 'vector', False, (0.2, 0.3, 0.5), 1e-3),
    'omni_lr_so_vector_K1_T1': ('omni', (0,), 1, 'lr', 'vector', False, (1.0,), 1e-3),
    'omni_lr_fo_per_step': ('omni', (0, 1, 2), 2, 'lr', 'per_step', True, (0.0, 1.0), 1e-3),
    'omni_lr_so_frozen_bias': ('omni', (1, 2, 3), 2, 'lr', 'frozen_bias', False, (0.0, 1.0), 1e-3),
    'omni3w2s_steps_so_per_step': ('omni3w2s', (0, 1), 2, 'steps', 'per_step', False, (0.3, 0.7), 1e-3),
    'min_steps_so_per_step': ('min', (0, 1), 2, 'steps', 'per_step', False, (0.3, 0.7), 2e-3),
    'min_lr_so_frozen_bias': ('min', (0, 1), 2, 'lr', 'frozen_bias', False, (0.0, 1.0), 2e-3),
}


def case_lr(case):
    shape, _, K, _, kind, _, _, _ = ORACLE_CASES[case]
    _, _, fc, ways, _ = SHAPES[shape][1:]
    if kind == 'scalar':
        return BASE_LR
    return lr_vector(fc, ways, BASE_LR, K if kind == 'per_step' else 1, 5, frozen=('bias',) if kind == 'frozen_bias' else ())


def case_oracle(case, dtype=torch.float64):
    shape, ids, K, _, _, fo, w, _ = ORACLE_CASES[case]
    base, tf, th, fc, ways, shots = fixtures(shape, dtype)
    datas, labels = tasks(shape, list(ids), dtype)
    return meta_batch(tf, th, base, fc, datas, labels, K, shots, ways, case_lr(case), w, fo, dtype)
