"""Oracle (TEST INFRASTRUCTURE) for the ridge-regression head (mi_ridge_head, mi_meta_batch_ridge): the definition
of R2-D2's head written out in torch with autograd through ``torch.linalg.solve`` (``head``), the fused call on oracle/vision_ref.py's
conv_base and prepare_batch exactly as tests/metric_head_oracle.py builds its features (``meta_batch``), and the closed form the kernel
implements, without autograd (``closed_form``), for the host test that pins one against the other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vision_ref as R
import anil_steps_oracle as A
import metric_head_oracle as M

SHAPES, fixtures, tasks, clear_rows, rel_err = A.SHAPES, A.fixtures, A.tasks, A.clear_rows, A.rel_err
kernel_inputs = M.kernel_inputs
GRAD_FLOOR, LOSS_FLOOR = M.GRAD_FLOOR, M.LOSS_FLOOR        # tests/test_gpu_anil.py's bars for the same trunks; 1e-4 on the loss
HYPER_FLOOR = 1e-4
EPS32 = float(np.finfo(np.float32).eps)

# The fused-call cases: shape -> (task ids, lam, alpha).  At alpha = 8 the `min` loss is 0.002 in fp64 (saturated): the values are part of
# the cases, and tests/test_ridge_head_host.py is what fixes them (loss inside [0.05, 3], at most one unclear row in ten).
FUSED_CASES = {
    'omni': ((0, 1, 2, 3), 1.0, 8.0),
    'omni3w2s': ((0, 1, 2), 1.0, 8.0),
    'min': ((0, 1, 2), 1.0, 1.0),
}

# ---- the kernel-entry cases: metric_head_oracle's (feat, ways, ns, nq, tasks) and Omniglot 20-way 5-shot, each under two (lam, alpha)
KERNEL_CASES = list(M.KERNEL_CASES) + [(128, 20, 100, 100, 1)]
HYPERS = [(1.0, 8.0), (50.0, 8.0)]
MAX_FEAT = 65536                                            # MI_RIDGE_MAX_FEAT


def lds_bytes(ns, nq, ways):
    """The kernel's LDS request in bytes, as include/mi_maml.h states it; the domain is lds_bytes <= 163840 (160 KiB)."""
    return 8 * (ns * (ns + 1) // 2 + nq * ns + 2 * ns * ways + ns + 3 * nq) + 4 * nq * ways


def logits_of(fs, fq, ys, ways, lam, alpha, bias=None):
    """[nq, ways] logits of one task from the definition; differentiable in fs, fq, lam, alpha (tensors) and the optional bias."""
    onehot = F.one_hot(ys.long(), ways).to(fs.dtype)                      # [ns, ways]
    g = fs @ fs.t() + lam * torch.eye(fs.shape[0], dtype=fs.dtype)
    z = alpha * ((fq @ fs.t()) @ torch.linalg.solve(g, onehot))
    return z if bias is None else z + bias


def _leaves(fs, fq, ys, yq, lam, alpha, dtype):
    fs = torch.as_tensor(np.asarray(fs)).to(dtype).clone().requires_grad_(True)
    fq = torch.as_tensor(np.asarray(fq)).to(dtype).clone().requires_grad_(True)
    ys, yq = torch.as_tensor(np.asarray(ys)).long(), torch.as_tensor(np.asarray(yq)).long()
    T = fs.shape[0]
    lams = torch.full((T,), float(lam), dtype=dtype, requires_grad=True)
    alphas = torch.full((T,), float(alpha), dtype=dtype, requires_grad=True)
    return fs, fq, ys, yq, lams, alphas


def head(fs, fq, ys, yq, ways, lam, alpha, dtype=torch.float64):
    """fs [T, ns, F], fq [T, nq, F], ys [T, ns], yq [T, nq] (arrays or tensors).  Returns numpy (loss [T], acc [T], logits [T, nq, ways],
    dfs, dfq, dhyper [T, 2] = (dloss_t/dlam, dloss_t/dalpha), cond [T]) with dfs, dfq the gradient of sum_t loss_t and cond the 2-norm
    condition number of G computed in fp64 whatever ``dtype``."""
    fs, fq, ys, yq, lams, alphas = _leaves(fs, fq, ys, yq, lam, alpha, dtype)
    losses, accs, logits, conds = [], [], [], []
    for t in range(fs.shape[0]):
        z = logits_of(fs[t], fq[t], ys[t], ways, lams[t], alphas[t])
        losses.append(F.cross_entropy(z, yq[t]))
        accs.append(float(R.accuracy(z, yq[t])))
        logits.append(z.detach())
        f64 = fs[t].detach().double()
        conds.append(float(np.linalg.cond((f64 @ f64.t() + float(lam) * torch.eye(f64.shape[0], dtype=torch.float64)).numpy())))
    torch.stack(losses).sum().backward()
    return (torch.stack(losses).detach().double().numpy(), np.asarray(accs), torch.stack(logits).double().numpy(),
            fs.grad.double().numpy(), fq.grad.double().numpy(), torch.stack([lams.grad, alphas.grad], dim=1).double().numpy(),
            np.asarray(conds))


def closed_form(fs, fq, ys, yq, ways, lam, alpha, dtype=torch.float64):
    """The formulas the kernel implements, no autograd; ``head``'s returns without cond."""
    fs, fq = torch.as_tensor(np.asarray(fs)).to(dtype), torch.as_tensor(np.asarray(fq)).to(dtype)
    ys, yq = torch.as_tensor(np.asarray(ys)).long(), torch.as_tensor(np.asarray(yq)).long()
    out = [[], [], [], [], [], []]
    for t in range(fs.shape[0]):
        s, q, nq = fs[t], fq[t], fq.shape[1]
        y = F.one_hot(ys[t], ways).to(dtype)
        g = s @ s.t() + lam * torch.eye(s.shape[0], dtype=dtype)
        a = torch.linalg.solve(g, y)
        k = q @ s.t()
        p = k @ a
        z = alpha * p
        lse = torch.logsumexp(z, dim=-1)
        loss = (lse - z.gather(1, yq[t][:, None])[:, 0]).mean()
        acc = (z.argmax(dim=-1) == yq[t]).to(dtype).mean()
        dz = (torch.softmax(z, dim=-1) - F.one_hot(yq[t], ways).to(dtype)) / nq
        dalpha = (dz * p).sum()
        dp = alpha * dz
        dk = dp @ a.t()
        da = k.t() @ dp
        b = torch.linalg.solve(g, da)
        sm = -(b @ a.t() + a @ b.t())
        dlam = -(b * a).sum()
        dfq = dk @ s
        dfs = dk.t() @ q + sm @ s
        for o, v in zip(out, (loss, acc, z, dfs, dfq, torch.stack([dlam, dalpha]))):
            o.append(v)
    return tuple(torch.stack(o).double().numpy() for o in out)


def bias_gradient(fs, fq, ys, yq, ways, lam, alpha):
    """d(sum_t loss_t)/dbeta of the variant with R2-D2's additive logit bias beta (a scalar), at beta = 0, in fp64."""
    fs, fq, ys, yq, lams, alphas = _leaves(fs, fq, ys, yq, lam, alpha, torch.float64)
    beta = torch.zeros((), dtype=torch.float64, requires_grad=True)
    total = sum(F.cross_entropy(logits_of(fs[t], fq[t], ys[t], ways, lams[t], alphas[t], bias=beta), yq[t]) for t in range(fs.shape[0]))
    total.backward()
    return float(beta.grad)


def meta_batch(theta_feat, base, fc, datas, labelss, shots, ways, lam, alpha, dtype=torch.float64):
    """The fused call: per task features = conv_base(data).view(-1, fc) on all 2n rows, prepare_batch's split, the ridge head on (support,
    query), the sum of the tasks' losses backward into the trunk.  Returns a dict of numpy arrays: losses [T], accs [T], logits [T, n,
    ways], grad_feat (flat, parameters() order), dhyper [T, 2]."""
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    leaves = list(fl.values())
    feats = lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc)
    T = len(datas)
    lams = torch.full((T,), float(lam), dtype=dtype, requires_grad=True)
    alphas = torch.full((T,), float(alpha), dtype=dtype, requires_grad=True)
    losses, accs, logits = [], [], []
    for t, (data, labels) in enumerate(zip(datas, labelss)):
        fs, ys, fq, yq = R.prepare_batch(data.to(dtype), labels, shots, ways, feats)
        z = logits_of(fs, fq, ys, ways, lams[t], alphas[t])
        loss = F.cross_entropy(z, yq)
        loss.backward()
        losses.append(float(loss.detach()))
        accs.append(float(R.accuracy(z, yq)))
        logits.append(z.detach().double().numpy())
    zero = lambda v: v.grad if v.grad is not None else torch.zeros_like(v)
    return dict(losses=np.asarray(losses), accs=np.asarray(accs), logits=np.asarray(logits),
                grad_feat=torch.cat([zero(v).reshape(-1) for v in leaves]).double().numpy(),
                dhyper=torch.stack([lams.grad, alphas.grad], dim=1).double().numpy())


def case_oracle(shape, ids=None, dtype=torch.float64):
    """meta_batch's dict of a fused-call case."""
    base, tf, _, fc, ways, shots = fixtures(shape, dtype)
    case_ids, lam, alpha = FUSED_CASES[shape]
    datas, labels = tasks(shape, list(case_ids if ids is None else ids), dtype)
    return meta_batch(tf, base, fc, datas, labels, shots, ways, lam, alpha, dtype)
