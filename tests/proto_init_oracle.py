"""Oracle (TEST INFRASTRUCTURE) for the Proto-MAML head initialisation (mi_proto_init, mi_proto_init_bwd, mi_meta_batch_anil_proto;
DESIGN.md section 30): ``meta_batch`` is tests/anil_steps_oracle.py's autograd restatement of the ANIL train half with the head's
parameters initialised from the support features INSIDE the graph (W_0 = 2 s c, b_0 = -s |c|^2, the scale a leaf), so that autograd alone
carries the gradient through the loop and through the initialisation; ``init_autograd`` is the same initialisation alone against a given
cotangent; ``init`` / ``init_bwd`` are the formulas the kernels implement, without autograd, for the host test that pins one against the
other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
import anil_steps_oracle as A
import metric_head_oracle as M

SHAPES, fixtures, tasks, clear_rows, rel_err, lr_vector, head_count = A.SHAPES, A.fixtures, A.tasks, A.clear_rows, A.rel_err, A.lr_vector, A.head_count
HEAD = A.HEAD

# shape -> (task ids, scale, inner step): metric_head_oracle.FUSED_CASES' proto scales; W_0 = 2 s c is large against a learned head, so the
# step is below anil_steps_oracle.BASE_LR, chosen on the fp64 oracle so that one step lowers the query loss by 1 to 10 per cent;
# tests/test_proto_init_host.py asserts on every fused case below that the fp64 loss of every (step, task) lies in [0.05, 3] and that at
# most one row in ten is under clear_rows' margin.
CASES = {
    'omni': ((0, 1, 2), 0.125, 0.2),
    'omni3w2s': ((0, 1), 0.125, 0.2),
    'min': ((0, 1), 2.0 ** -8, 2.0 ** -7),
}
FUSED_CASES = CASES                  # (closed_form_utils.inputs reads the task ids from here)
GRAD_FLOOR = M.GRAD_FLOOR            # tests/test_gpu_anil.py's bars for the same trunks
LOSS_FLOOR = 1e-4

# name: shape, task ids (None: the shape's), K, step ('scalar' / 'vector' / 'per_step'), first order, weights (None: the final loss)
FUSED = {
    'omni_K0': ('omni', None, 0, 'scalar', False, None),
    'omni_K1_so_scalar': ('omni', None, 1, 'scalar', False, None),
    'omni_K3_so_steps_scalar': ('omni', None, 3, 'scalar', False, (0.2, 0.3, 0.5)),
    'omni_K2_so_per_step': ('omni', None, 2, 'per_step', False, None),
    'omni_K2_fo_vector': ('omni', None, 2, 'vector', True, None),
    'omni_K2_so_steps_T1': ('omni', (1,), 2, 'scalar', False, (0.3, 0.7)),
    'omni3w2s_K2_so': ('omni3w2s', None, 2, 'scalar', False, None),
    'min_K2_so': ('min', None, 2, 'scalar', False, None),
}


def case_ids(case):
    shape, ids = FUSED[case][:2]
    return list(CASES[shape][0] if ids is None else ids)


def case_lr(case):
    """The scalar step of the case's shape, or the [steps, Ph] vector around it (anil_steps_oracle.lr_vector, seed 5)."""
    shape, _, K, kind, _, _ = FUSED[case]
    _, _, fc, ways, _ = SHAPES[shape][1:]
    step = CASES[shape][2]
    return step if kind == 'scalar' else lr_vector(fc, ways, step, K if kind == 'per_step' else 1, 5)


def head_init(fs, ys, ways, scale):
    """(W_0 [ways, F], b_0 [ways]) of one task from the definition; differentiable in fs and scale.  A class without a support row is outside
    the definition; it is treated as include/mi_maml.h states (c_w = 0: W_0 = 0, b_0 = 0, no gradient), which changes nothing for N_w >= 1."""
    onehot = F.one_hot(ys.long(), ways).to(fs.dtype)
    c = (onehot.t() @ fs) / onehot.sum(dim=0).clamp(min=1)[:, None]
    return 2 * scale * c, -scale * (c * c).sum(dim=-1)


def meta_batch(theta_feat, base, fc, datas, labelss, K, shots, ways, scale, lr, step_w, first_order, dtype=torch.float64, detach_init=False):
    """anil_steps_oracle.meta_batch with p = head_init(support features, scale) inside the graph.  step_w None: the objective is the loss
    at theta_K.  detach_init: theta_0 a constant (what first order must NOT be).  Returns a dict of numpy arrays: losses, accs [K + 1, T],
    logits [K + 1, T, n, ways], grad_feat (flat, parameters() order), lr_grad [steps, Ph] or None, dscale (summed), dscale_tasks [T]."""
    so = not first_order
    T = len(datas)
    w = [0.0] * (K - 1) + [1.0] * min(K, 1) if step_w is None else [float(x) for x in np.asarray(step_w, dtype=np.float64)]
    assert len(w) == K
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    s = torch.tensor(float(scale), dtype=dtype, requires_grad=True)
    lrs = None if A._is_scalar(lr) else A._lr_leaves(lr, fc, ways, dtype)
    feats = lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc)
    losses, accs, logits = np.zeros((K + 1, T)), np.zeros((K + 1, T)), [[None] * T for _ in range(K + 1)]
    dscale_tasks, seen = np.zeros(T), 0.0
    for t, (data, labels) in enumerate(zip(datas, labelss)):
        ad, al, ed, el = R.prepare_batch(data.to(dtype), labels, shots, ways, feats)
        w0, b0 = head_init(ad, al, ways, s)
        p = OrderedDict((('weight', w0.detach() if detach_init else w0), ('bias', b0.detach() if detach_init else b0)))
        if detach_init:
            p = OrderedDict((n, v.requires_grad_(True)) for n, v in p.items())
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
            step = (lambda n: float(lr)) if lrs is None else (lambda n: A._row(lrs, n, j))
            p = OrderedDict((n, v - step(n) * g) for (n, v), g in zip(p.items(), gs))
        (objective if K >= 1 else lq).backward()
        total = float(s.grad) if s.grad is not None else 0.0
        dscale_tasks[t], seen = total - seen, total
    zero = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
    lg = None
    if lrs is not None:
        steps = lrs['weight'].shape[0]
        lg = torch.cat([zero(lrs[n]).reshape(steps, -1) for n in HEAD], dim=1).double().numpy()
    return dict(losses=losses, accs=accs, logits=np.asarray(logits), grad_feat=A._flat([zero(v) for v in fl.values()]).double().numpy(),
                lr_grad=lg, dscale=float(dscale_tasks.sum()), dscale_tasks=dscale_tasks)


def case_oracle(case, dtype=torch.float64):
    shape, _, K, _, fo, w = FUSED[case]
    base, tf, _, fc, ways, shots = fixtures(shape, dtype)
    datas, labels = tasks(shape, case_ids(case), dtype)
    return meta_batch(tf, base, fc, datas, labels, K, shots, ways, CASES[shape][1], case_lr(case), w, fo, dtype)


# ---- the initialisation alone: [T, ways * F + ways] per task, W_0 row-major then b_0
def init_autograd(fs, ys, lam, ways, scale, dtype=torch.float64):
    """head [T, Ph], and against the cotangent lam [T, Ph]: dfs [T, ns, F], dscale [T], all by autograd; numpy."""
    fs = torch.as_tensor(np.asarray(fs)).to(dtype).clone().requires_grad_(True)
    ys = torch.as_tensor(np.asarray(ys)).long()
    lam = torch.as_tensor(np.asarray(lam)).to(dtype)
    heads, dscale = [], []
    for t in range(fs.shape[0]):
        s = torch.tensor(float(scale), dtype=dtype, requires_grad=True)
        w0, b0 = head_init(fs[t], ys[t], ways, s)
        h = torch.cat([w0.reshape(-1), b0])
        (h * lam[t]).sum().backward()
        heads.append(h.detach())
        dscale.append(s.grad)
    return torch.stack(heads).double().numpy(), fs.grad.double().numpy(), torch.stack(dscale).double().numpy()


def init(fs, ys, ways, scale):
    """The forward kernel's formulas in fp64 numpy: [T, ways * F + ways]."""
    fs, ys = np.asarray(fs, dtype=np.float64), np.asarray(ys)
    T, _, feat = fs.shape
    out = np.zeros((T, ways * feat + ways))
    for t in range(T):
        for w in range(ways):
            c = fs[t][ys[t] == w].sum(axis=0) / (ys[t] == w).sum()
            out[t, w * feat:(w + 1) * feat] = 2 * scale * c
            out[t, ways * feat + w] = -scale * (c * c).sum()
    return out


def init_bwd(fs, ys, lam, ways, scale, dfs0=None):
    """The backward kernel's formulas in fp64 numpy: (dfs0 + the gradient through the initialisation, dscale [T])."""
    fs, ys, lam = np.asarray(fs, dtype=np.float64), np.asarray(ys), np.asarray(lam, dtype=np.float64)
    T, _, feat = fs.shape
    dfs = np.zeros_like(fs) if dfs0 is None else np.asarray(dfs0, dtype=np.float64).copy()
    dscale = np.zeros(T)
    for t in range(T):
        for w in range(ways):
            rows = ys[t] == w
            c = fs[t][rows].sum(axis=0) / rows.sum()
            lw, lb = lam[t, w * feat:(w + 1) * feat], lam[t, ways * feat + w]
            dfs[t][rows] += 2 * scale * (lw - lb * c) / rows.sum()
            dscale[t] += 2 * (lw * c).sum() - lb * (c * c).sum()
    return dfs, dscale


# ---- the kernel-entry cases: (feat, ways, ns, tasks); metric_head_oracle.kernel_inputs' features, a hash-uniform cotangent in [-1, 1)
KERNEL_CASES = [(1, 5, 5, 1), (33, 5, 5, 1), (128, 5, 5, 3), (1600, 5, 25, 2), (128, 1, 3, 1), (128, 20, 20, 1), (128, 3, 6, 1), (128, 20, 100, 1),
                (8, 64, 64, 1)]
# the paths no case above runs: stride 4 * 1028 + 4 = 4116, a multiple of 4, so the 16-byte forward loop wraps past column 1024 and the vector
# backward has 1028 items (> 512); a partial last chunk (nv = 3) after the wrap with class counts (1, 2, 3); classes 1 and 3 without a
# support row (metric_head_oracle.ABSENT) on odd feat > 512
EDGE_CASES = [(1028, 4, 8, 1), (1027, 3, 6, 1), (515, 5, 3, 1)]
MAX_FEAT = 65536                     # MI_RIDGE_MAX_FEAT


def kernel_inputs(feat, ways, ns, T):
    """(fs, ys, lam [T, Ph], dfs0 [T, ns, feat]) numpy; (3 ways, 6 rows) has the class counts 1, 2 and 3."""
    fs, _, ys, _ = M.kernel_inputs(feat, ways, ns, ns, T)
    lam = (2.0 * synthetic.hash_uniform(37, (T, ways * feat + ways)) - 1.0).astype(np.float32)
    dfs0 = (2.0 * synthetic.hash_uniform(41, (T, ns, feat)) - 1.0).astype(np.float32)
    return fs, ys, lam, dfs0
