"""Oracle (TEST INFRASTRUCTURE) for the metric heads (mi_metric_head, mi_meta_batch_metric): the definitions of
Prototypical Networks and NIL written out in torch with autograd (``head``), the fused call on oracle/vision_ref.py's conv_base and
prepare_batch exactly as tests/anil_steps_oracle.py builds its features (``meta_batch``), and the closed form the kernel implements,
without autograd (``closed_form``), for the host test that pins one against the other."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vision_ref as R
import anil_steps_oracle as A

SHAPES, fixtures, tasks, clear_rows, rel_err = A.SHAPES, A.fixtures, A.tasks, A.clear_rows, A.rel_err
PROTO, COSINE = 'proto', 'cosine'
EPS = 1e-8

# The fused-call cases: shape -> (task ids, proto scale, cosine scale).  At scale 1 the `min` proto logits reach -600 and the loss and its
# gradient are exactly 0 in fp64: the scales are part of the cases.
FUSED_CASES = {
    'omni': ((0, 1, 2, 3), 0.125, 4.0),
    'omni3w2s': ((0, 1, 2), 0.125, 4.0),
    'min': ((0, 1, 2), 2.0 ** -8, 1.0),
}
GRAD_FLOOR = {'omni': 1e-3, 'omni3w2s': 1e-3, 'min': 2e-3}      # tests/test_gpu_anil.py's bars for the same trunks
LOSS_FLOOR = 1e-4


def case_scale(shape, metric):
    return FUSED_CASES[shape][1 if metric == PROTO else 2]


def _normalise(x):
    """x / max(|x|_2, 1e-8) by hand (F.cosine_similarity clamps differently between torch versions)."""
    return x / x.norm(dim=-1, keepdim=True).clamp(min=EPS)


def logits_of(fs, fq, ys, ways, metric, scale):
    """[nq, ways] logits of one task from the definitions; differentiable in fs and fq."""
    onehot = F.one_hot(ys.long(), ways).to(fs.dtype)                      # [ns, ways]
    if metric == PROTO:
        c = (onehot.t() @ fs) / onehot.sum(dim=0)[:, None]
        return -scale * ((fq[:, None, :] - c[None, :, :]) ** 2).sum(dim=-1)
    if metric == COSINE:
        c = onehot.t() @ _normalise(fs)
        return scale * (_normalise(fq) @ c.t())
    raise ValueError(metric)


def head(fs, fq, ys, yq, ways, metric, scale, dtype=torch.float64):
    """fs [T, ns, F], fq [T, nq, F], ys [T, ns], yq [T, nq] (arrays or tensors).  Returns numpy (loss [T], acc [T], logits [T, nq, ways],
    dfs, dfq) with dfs, dfq the gradient of sum_t loss_t."""
    fs = torch.as_tensor(np.asarray(fs)).to(dtype).clone().requires_grad_(True)
    fq = torch.as_tensor(np.asarray(fq)).to(dtype).clone().requires_grad_(True)
    ys, yq = torch.as_tensor(np.asarray(ys)).long(), torch.as_tensor(np.asarray(yq)).long()
    losses, accs, logits = [], [], []
    for t in range(fs.shape[0]):
        z = logits_of(fs[t], fq[t], ys[t], ways, metric, scale)
        losses.append(F.cross_entropy(z, yq[t]))
        accs.append(float(R.accuracy(z, yq[t])))
        logits.append(z.detach())
    torch.stack(losses).sum().backward()
    return (torch.stack(losses).detach().double().numpy(), np.asarray(accs), torch.stack(logits).double().numpy(),
            fs.grad.double().numpy(), fq.grad.double().numpy())


def closed_form(fs, fq, ys, yq, ways, metric, scale, dtype=torch.float64):
    """The formulas the kernel implements, no autograd; same returns as ``head``."""
    fs, fq = torch.as_tensor(np.asarray(fs)).to(dtype), torch.as_tensor(np.asarray(fq)).to(dtype)
    ys, yq = torch.as_tensor(np.asarray(ys)).long(), torch.as_tensor(np.asarray(yq)).long()
    out = [[], [], [], [], []]
    for t in range(fs.shape[0]):
        s, q, nq = fs[t], fq[t], fq.shape[1]
        onehot = F.one_hot(ys[t], ways).to(dtype)
        counts = onehot.sum(dim=0)
        if metric == PROTO:
            c = (onehot.t() @ s) / counts[:, None]
            diff = q[:, None, :] - c[None, :, :]                           # [nq, ways, F]
            z = -scale * (diff ** 2).sum(dim=-1)
        else:
            ns_, nq_ = s.norm(dim=-1, keepdim=True), q.norm(dim=-1, keepdim=True)
            sh, qh = s / ns_.clamp(min=EPS), q / nq_.clamp(min=EPS)
            c = onehot.t() @ sh
            z = scale * (qh @ c.t())
        lse = torch.logsumexp(z, dim=-1)
        loss = (lse - z.gather(1, yq[t][:, None])[:, 0]).mean()
        acc = (z.argmax(dim=-1) == yq[t]).to(dtype).mean()
        dz = (torch.softmax(z, dim=-1) - F.one_hot(yq[t], ways).to(dtype)) / nq
        if metric == PROTO:
            dfq = -2 * scale * (dz[:, :, None] * diff).sum(dim=1)
            dc = 2 * scale * (dz[:, :, None] * diff).sum(dim=0)
            dfs = dc[ys[t]] / counts[ys[t]][:, None]
        else:
            def through(dxh, xh, nrm):
                proj = (dxh - (dxh * xh).sum(dim=-1, keepdim=True) * xh) / nrm.clamp(min=EPS)
                return torch.where(nrm >= EPS, proj, dxh / EPS)
            dfq = through(scale * (dz @ c), qh, nq_)
            dc = scale * (dz.t() @ qh)
            dfs = through(dc[ys[t]], sh, ns_)
        for o, v in zip(out, (loss, acc, z, dfs, dfq)):
            o.append(v)
    return tuple(torch.stack(o).double().numpy() for o in out)


def meta_batch_heads(theta_feat, base, fc, datas, labelss, shots, ways, heads, dtype=torch.float64):
    """``meta_batch`` for several (metric, scale) heads on ONE trunk pass per task (the trunk is the oracle's whole cost): a list of
    ``meta_batch``'s dicts, one per head."""
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    leaves = list(fl.values())
    feats = lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc)
    outs = [dict(losses=[], accs=[], logits=[], grad_feat=[torch.zeros_like(v) for v in leaves]) for _ in heads]
    for data, labels in zip(datas, labelss):
        fs, ys, fq, yq = R.prepare_batch(data.to(dtype), labels, shots, ways, feats)
        for o, (metric, scale) in zip(outs, heads):
            z = logits_of(fs, fq, ys, ways, metric, scale)
            loss = F.cross_entropy(z, yq)
            for acc, g in zip(o['grad_feat'], torch.autograd.grad(loss, leaves, retain_graph=True, allow_unused=True)):
                if g is not None:
                    acc += g
            o['losses'].append(float(loss.detach()))
            o['accs'].append(float(R.accuracy(z, yq)))
            o['logits'].append(z.detach().double().numpy())
    return [dict(losses=np.asarray(o['losses']), accs=np.asarray(o['accs']), logits=np.asarray(o['logits']),
                 grad_feat=torch.cat([g.reshape(-1) for g in o['grad_feat']]).double().numpy()) for o in outs]


def meta_batch(theta_feat, base, fc, datas, labelss, shots, ways, metric, scale, dtype=torch.float64):
    """The fused call: per task features = conv_base(data).view(-1, fc) on all 2n rows, prepare_batch's split, the metric head on
    (support, query), the sum of the tasks' losses backward into the trunk.  Returns a dict of numpy arrays: losses [T], accs [T],
    logits [T, n, ways], grad_feat (flat, parameters() order)."""
    return meta_batch_heads(theta_feat, base, fc, datas, labelss, shots, ways, [(metric, scale)], dtype)[0]


def case_oracle(shape, ids=None, dtype=torch.float64):
    """{metric: meta_batch's dict} of a fused-call case, both metrics from one trunk pass per task."""
    base, tf, _, fc, ways, shots = fixtures(shape, dtype)
    datas, labels = tasks(shape, list(FUSED_CASES[shape][0] if ids is None else ids), dtype)
    heads = [(m, case_scale(shape, m)) for m in (PROTO, COSINE)]
    return dict(zip((PROTO, COSINE), meta_batch_heads(tf, base, fc, datas, labels, shots, ways, heads, dtype)))


# ---- the kernel-entry cases: (feat, ways, ns, nq, tasks); features hash_uniform scaled to [0, 3], the trunk's range
KERNEL_CASES = [(1, 5, 5, 5, 1), (33, 5, 5, 5, 1), (128, 5, 5, 5, 3), (1600, 5, 25, 25, 2), (128, 1, 3, 3, 1), (128, 20, 20, 20, 1),
                (128, 3, 6, 4, 1)]


def balanced_labels(n, ways):
    """n labels in [0, ways), classes ascending, every class present (n >= ways)."""
    return (np.arange(n) * ways // n).astype(np.int32)


# the paths no case above runs: 64 classes on odd feat > 512 (lanes 32..63, eight chunks of 8 classes and dfq's read-modify-write over them, the
# scalar loops past one trip; 37848 of 40960 LDS floats), exactly one chunk of 8 classes and one class into the second, nq > 64, nq = 1
EDGE_CASES = [(515, 64, 64, 70, 1), (128, 8, 8, 8, 1), (128, 9, 9, 9, 1), (515, 5, 5, 75, 2), (4, 2, 2, 1, 1)]
# (ways, ns) -> the support labels of the cases with ns < ways: classes 1 and 3 have no support row (legal for the ridge head; W_0 = 0, b_0 = 0
# and no gradient in the Proto-MAML initialisation; outside the metric heads' contract).  (2, 1): the one support row is of class 1 and the
# one query row of class 0 -- with the support row in class 0 the ridge head's fp64 loss is 9.7e-4 at (lam, alpha) = (1, 8), under the 1e-3
# a case must have for a relative bar on it to mean something (tests/test_ridge_head_host.py)
ABSENT = {(5, 3): (0, 2, 4), (2, 1): (1,)}


def kernel_inputs(feat, ways, ns, nq, T, seed=31, ys=None):
    """(fs, fq, ys, yq) numpy; (3 ways, 6 support rows) is the unbalanced case with class counts 1, 2 and 3; ys: the support labels of one
    task, given explicitly (default: ABSENT's where ns < ways says so, else balanced)."""
    from exploring_meta_amd.utils import synthetic
    fs = (3.0 * synthetic.hash_uniform(seed, (T, ns, feat))).astype(np.float32)
    fq = (3.0 * synthetic.hash_uniform(seed + 1, (T, nq, feat))).astype(np.float32)
    ys = ABSENT.get((ways, ns)) if ys is None else ys
    if ys is not None:
        ys = np.asarray(ys, np.int32)
        assert ys.shape == (ns,) and ys.min() >= 0 and ys.max() < ways
    else:
        ys = np.array([0, 1, 1, 2, 2, 2], np.int32) if (ways, ns) == (3, 6) else balanced_labels(ns, ways)
    yq = (np.arange(nq) % ways).astype(np.int32)
    return fs, fq, np.tile(ys, (T, 1)), np.tile(yq, (T, 1))


def lds_floats(ns, nq, feat, ways):
    """The kernel's LDS request in floats, as include/mi_maml.h states it; the domain is lds_floats <= 40960 (160 KiB)."""
    return (ways * feat + 3) // 4 * 4 + nq * ways + ways + ns + 4 * nq
