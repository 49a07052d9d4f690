"""Oracle (TEST INFRASTRUCTURE) for the ridge-regression head (mi_ridge_head, mi_meta_batch_ridge): the definition
of R2-D2's head written out in torch with autograd through ``torch.linalg.solve`` (``head``), the fused call on oracle/vision_ref.py's
conv_base and prepare_batch exactly as tests/metric_head_oracle.py builds its features (``meta_batch``), and the closed form the kernel
implements, without autograd (``closed_form``), for the host test that pins one against the other; the same closed form in NumPy at a chosen precision (``closed_form_np``), which in
``np.longdouble`` is the extended-precision reference (``closed_form_ext``) the kernel's fp64 claim is held to (``tight_errors``), and in
fp64 with fp32 stores the host's model of the kernel."""
import hashlib
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
# the paths no case above runs: 64 ways on odd feat > 512 (lanes 32..63, rstep = 8, the scalar loops past one trip, 138128 bytes of LDS: the
# dynamic-LDS attribute); ns < ways with absent classes (metric_head_oracle.ABSENT's labels) and nq > 64; ns = nq = 1 on one vector chunk;
# one class, ns = 1 on one scalar chunk
EDGE_CASES = [(515, 64, 64, 70, 1), (515, 5, 3, 75, 2), (4, 2, 1, 1, 1), (5, 1, 1, 3, 1)]
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


# ---- the closed form in NumPy at a chosen precision: np.longdouble (the x87 80-bit format, eps = 2^-63) is the reference the kernel's
# fp64 claim is held to; there is no LAPACK for that type, so the factor and the substitutions are written out (sizes are at most 100 x 100)
def ldl(g):
    """G = L D L^T in g's own dtype, no pivoting: (L, unit lower triangular; d, the pivots).  A pivot that is not > 0 is returned as it is
    (the column under it is then not finite)."""
    n = g.shape[0]
    low, d = np.eye(n, dtype=g.dtype), np.zeros(n, dtype=g.dtype)
    with np.errstate(all='ignore'):
        for j in range(n):
            v = low[j, :j] * d[:j]
            d[j] = g[j, j] - low[j, :j] @ v
            low[j + 1:, j] = (g[j + 1:, j] - low[j + 1:, :j] @ v) / d[j]
    return low, d


def ldl_solve(low, d, x):
    """G^-1 X from ``ldl``'s factor: forward, diagonal and backward substitution."""
    x = x.copy()
    n = x.shape[0]
    for k in range(1, n):
        x[k] -= low[k, :k] @ x[:k]
    x /= d[:, None]
    for k in range(n - 2, -1, -1):
        x[k] -= low[k + 1:, k] @ x[k + 1:]
    return x


_CACHE = {}


def _key(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str((a.dtype, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _products(s32, q32, dtype):
    """(Fs Fs^T, Fq Fs^T) of one task in ``dtype``; the longdouble products, the slow part, are kept: every (lam, alpha) reuses them."""
    if dtype is not np.longdouble:
        s, q = s32.astype(dtype), q32.astype(dtype)
        return s @ s.T, q @ s.T
    key = ('products', _key(s32, q32))
    if key not in _CACHE:
        s, q = s32.astype(dtype), q32.astype(dtype)
        _CACHE[key] = (s @ s.T, q @ s.T)
    return _CACHE[key]


def closed_form_np(fs, fq, ys, yq, ways, lam, alpha, dtype=np.float64, round_dp=False, gram_dtype=None, round_out=False):
    """``closed_form`` in NumPy with every intermediate in ``dtype`` and the hand-written ``ldl`` / ``ldl_solve``; lam and alpha are the
    fp32 values the C entry receives.  round_dp: dP = alpha dz is rounded to fp32 where the kernel stores it.  gram_dtype: Fs Fs^T is
    accumulated in that type instead (np.float32: the regression the header rules out).  round_out: loss, logits, dfs, dfq and dhyper are
    rounded to fp32 as a store does.  Returns ``closed_form``'s tuple as ``dtype`` arrays."""
    fs, fq = np.asarray(fs, dtype=np.float32), np.asarray(fq, dtype=np.float32)
    ys, yq = np.asarray(ys), np.asarray(yq)
    lam, alpha = dtype(np.float32(lam)), dtype(np.float32(alpha))
    T, ns, _ = fs.shape
    nq = fq.shape[1]
    out = [[], [], [], [], [], []]
    for t in range(T):
        s, q = fs[t].astype(dtype), fq[t].astype(dtype)
        gram, k = _products(fs[t], fq[t], dtype)
        if gram_dtype is not None:
            gram = (fs[t].astype(gram_dtype) @ fs[t].astype(gram_dtype).T).astype(dtype)
        y = (ys[t][:, None] == np.arange(ways)[None, :]).astype(dtype)
        hit = yq[t][:, None] == np.arange(ways)[None, :]
        low, d = ldl(gram + lam * np.eye(ns, dtype=dtype))
        a = ldl_solve(low, d, y)
        p = k @ a
        z = alpha * p
        mx = z.max(axis=-1, keepdims=True)
        ex = np.exp(z - mx)
        se = ex.sum(axis=-1, keepdims=True)
        loss = ((mx + np.log(se))[:, 0] - z[hit]).sum() / nq
        acc = dtype((z.argmax(axis=-1) == yq[t]).mean())
        dz = (ex / se - hit.astype(dtype)) / nq
        dalpha = (dz * p).sum()
        dp = alpha * dz
        if round_dp:
            dp = dp.astype(np.float32).astype(dtype)
        dk = dp @ a.T
        b = ldl_solve(low, d, k.T @ dp)
        sm = -(b @ a.T + a @ b.T)
        dlam = -(b * a).sum()
        for o, v in zip(out, (loss, acc, z, dk.T @ q + sm @ s, dk @ s, np.array([dlam, dalpha], dtype=dtype))):
            o.append(v)
    res = tuple(np.asarray(o, dtype=dtype) for o in out)
    if round_out:
        res = tuple(r if i == 1 else r.astype(np.float32).astype(dtype) for i, r in enumerate(res))
    return res


def closed_form_ext(fs, fq, ys, yq, ways, lam, alpha, round_dp):
    """The closed form the kernel implements in np.longdouble: the reference of ``tight_errors``.  One run per (inputs, lam, alpha,
    round_dp), kept and never modified."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, 'np.longdouble is not an extended format here: the ridge reference needs 64 bits of mantissa'
    key = ('ext', _key(np.asarray(fs, np.float32), np.asarray(fq, np.float32), np.asarray(ys, np.int64), np.asarray(yq, np.int64)), int(ways),
           float(np.float32(lam)), float(np.float32(alpha)), bool(round_dp))
    if key not in _CACHE:
        res = closed_form_np(fs, fq, ys, yq, ways, lam, alpha, np.longdouble, round_dp=round_dp)
        for r in res:
            r.setflags(write=False)
        _CACHE[key] = res
    return _CACHE[key]


# ---- the bar that holds the kernel to its fp64 claim; every term comes from references, none from the code under test
QUANTITIES = ('loss', 'logits', 'dfs', 'dfq', 'dlam', 'dalpha')
ROWWISE = ('logits', 'dfs', 'dfq')              # held per row as well: rows of nq, ns, nq
ULP32 = 2.0 ** -23


def quantities(o):
    """{name: array} of a (loss, acc, logits, dfs, dfq, dhyper, ...) tuple."""
    return dict(loss=o[0], logits=o[2], dfs=o[3], dfq=o[4], dlam=o[5][:, 0], dalpha=o[5][:, 1])


def rel_ext(a, b, rows=False):
    """|a - b| / |b| in np.longdouble, over everything or per row of the last axis; a zero reference divides by 1e-300 as ``rel_err``."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    if rows:
        a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        return (np.sqrt(((a - b) ** 2).sum(axis=-1)) / np.maximum(np.sqrt((b ** 2).sum(axis=-1)), 1e-300)).astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def tight_errors(got, o64, fs, fq, ys, yq, ways, lam, alpha):
    """{name: (error, bar)} for QUANTITIES and {name + '_rows': (errors, bars)} for ROWWISE.  The error is relative in norm against
    closed_form_ext(round_dp=False); the bar is 2^-23 + 2 e_dp + 2 e64 with
      e_dp = rel(closed_form_ext(round_dp=True), closed_form_ext(round_dp=False)): what the kernel's one stated fp32 intermediate may cost
             (0 for loss, logits and dalpha),
      e64  = rel(o64, closed_form_ext(round_dp=False)), o64 = head(..., float64): the fp64 reference's own distance from the truth,
      2^-23 one fp32 ulp: the output's own rounding takes half, device exp / log and the order of the fp64 sums the other half."""
    ext = quantities(closed_form_ext(fs, fq, ys, yq, ways, lam, alpha, False))
    ext_dp = quantities(closed_form_ext(fs, fq, ys, yq, ways, lam, alpha, True))
    got, o64 = quantities(got), quantities(o64)
    res = {}
    for n in QUANTITIES:
        for rows in ((False, True) if n in ROWWISE else (False,)):
            err, e_dp, e64 = (rel_ext(x[n], ext[n], rows) for x in (got, ext_dp, o64))
            res[n + '_rows' if rows else n] = (err, ULP32 + 2 * e_dp + 2 * e64)
    return res


# ---- the non-positive pivot: lam = 2^-80 is inside the domain (positive, finite, a normal fp32) and vanishes against G_ii = 4 in fp64
PIVOT_LAM = 2.0 ** -80


def pivot_inputs(plant_nan=False):
    """(fs, fq, ys, yq) of the (feat 4, ways 2, ns 2, nq 2) case at T = 3 whose task 1 has two support rows of all 1.0: G = [[4, 4], [4, 4]] +
    lam I rounds to [[4, 4], [4, 4]] at PIVOT_LAM, so the second pivot is exactly 0; tasks 0 and 2 keep their random features.  plant_nan:
    one element of task 1's fs is NaN as well."""
    fs, fq, ys, yq = kernel_inputs(4, 2, 2, 2, 3)
    fs[1] = 1.0
    if plant_nan:
        fs[1, 1, 2] = np.nan
    return fs, fq, ys, yq


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
