"""Oracle (TEST INFRASTRUCTURE) for the logistic-regression head (mi_logreg_head, mi_meta_batch_logreg): L2-regularised
multinomial logistic regression on the support features, solved to optimality in the dual form and differentiated through the optimum.
Two independent fp64 references and the fused form:
  ``head``         the definition: a damped Newton iteration with a dense ``torch.linalg.solve`` on the dual residual R(A) = lam A + softmax(G A)
                   - Y to |R|_inf <= 1e-13, then autograd through two further undamped Newton steps from the converged point (at R = 0 one
                   differentiable Newton step carries the implicit-function gradient exactly);
  ``closed_form``  the formulas and the solver the kernel implements, in NumPy, no autograd: Newton with the rank-reduced conjugate-gradient
                   solve of (lam I + D G), the acceptance rules, the implicit backward.  Also returns the Newton, CG and halving counts and the
                   final residual.  With round_out / gram_dtype / stop, accept it is the host's model of the kernel and its two mutants;
  ``meta_batch``   the fused call on oracle/vision_ref.py's conv_base and prepare_batch, as tests/ridge_head_oracle.py builds it."""
import os
import re
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

# The fused-call cases: shape -> (task ids, lam, alpha); tests/test_logreg_head_host.py is what fixes the values (fp64 loss inside [0.05, 3], no
# query row under clear_rows' margin).  At alpha = 1 the `min` loss is 0.008 at lam = 1 (saturated): the values are part of the cases.
FUSED_CASES = {
    'omni': ((0, 1, 2, 3), 1.0, 1.0),
    'omni3w2s': ((0, 1, 2), 1.0, 1.0),
    'min': ((0, 1, 2), 1.0, 0.25),
}

# ---- the kernel-entry cases: metric_head_oracle's (feat, ways, ns, nq, tasks), each under two (lam, alpha)
KERNEL_CASES = list(M.KERNEL_CASES)
# the paths no case above runs: 36 ways on odd feat > 512 (classes and first maxima in lanes 32..63, the scalar loops past one trip, 138880
# bytes of LDS: the dynamic-LDS attribute); ns < ways with absent classes (metric_head_oracle.ABSENT's labels) and nq > 64; ns = nq = 1 on one
# vector chunk; one class, ns = 1 on one scalar chunk; one feature, where G has rank 1
EDGE_CASES = [(515, 36, 36, 40, 1), (515, 5, 3, 75, 2), (4, 2, 1, 1, 1), (5, 1, 1, 3, 1), (1, 5, 5, 5, 1)]
ALL_CASES = KERNEL_CASES + [c for c in EDGE_CASES if c not in KERNEL_CASES]
HYPERS = [(1.0, 1.0), (50.0, 1.0)]
MAX_FEAT = 65536                                            # MI_RIDGE_MAX_FEAT

# ---- the solver's constants: the stopping rules compare quantities that do not change when the features are doubled and lam quadrupled
STOP, ACCEPT, CG_TOL, ARMIJO = 1e-13, 1e-10, 1e-13, 1e-4


def caps():
    """{'newton', 'cg', 'halve'}: the solver's compile-time caps, read from include/mi_maml.h."""
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'mi_maml.h')).read()
    return {k: int(re.search(r'#define MI_LOGREG_' + k.upper() + r'_CAP (\d+)', header).group(1)) for k in ('newton', 'cg', 'halve')}


def lds_bytes(ns, nq, ways):
    """The kernel's LDS request in bytes, as include/mi_maml.h states it; the domain is lds_bytes <= 163840 (160 KiB)."""
    return 8 * (ns * ns + nq * ns + 10 * ns * ways + nq * ways + 2 * ns + 3 * nq + 32)


# ------------------------------------------------------------------------------------------------------------------ reference 1: the definition
def _dual_residual(g, a, y, lam):
    return lam * a + torch.softmax(g @ a, dim=-1) - y


def _dual_jacobian(g, a, lam):
    """d vec(R) / d vec(A), dense [ns ways, ns ways]: lam I + D G with D_i = diag(p_i) - p_i p_i^T acting on row i."""
    ns, ways = a.shape
    p = torch.softmax(g @ a, dim=-1)
    d = torch.diag_embed(p) - p[:, :, None] * p[:, None, :]                 # [ns, ways, ways]
    return lam * torch.eye(ns * ways, dtype=a.dtype) + torch.einsum('icd,ij->icjd', d, g).reshape(ns * ways, ns * ways)


def _newton_step(g, a, y, lam):
    return a - torch.linalg.solve(_dual_jacobian(g, a, lam), _dual_residual(g, a, y, lam).reshape(-1)).reshape(a.shape)


def _objective(g, a, ys, lam):
    s = g @ a
    return float((torch.logsumexp(s, dim=-1) - s.gather(1, ys[:, None])[:, 0]).sum() + 0.5 * lam * (a * s).sum())


def solve_dual(g, ys, ways, lam, iters=200):
    """A* [ns, ways] with lam A + softmax(G A) = onehot(ys), fp64, no autograd: Newton with a dense solve, the step halved until it lowers
    |R|_inf or meets Armijo's condition on the inner objective."""
    y = F.one_hot(ys, ways).to(g.dtype)
    a = torch.zeros_like(y)
    with torch.no_grad():
        for _ in range(iters):
            r = _dual_residual(g, a, y, lam)
            rn = float(r.abs().max())
            if rn <= STOP:
                break
            step_dir = _newton_step(g, a, y, lam) - a
            slope = float(((g @ r) * step_dir).sum())
            f0, t, moved = _objective(g, a, ys, lam), 1.0, False
            for _ in range(60):
                cand = a + t * step_dir
                if float(_dual_residual(g, cand, y, lam).abs().max()) < rn or _objective(g, cand, ys, lam) <= f0 + ARMIJO * t * slope:
                    a, moved = cand, True
                    break
                t *= 0.5
            if not moved:
                break
        assert float(_dual_residual(g, a, y, lam).abs().max()) <= 1e-12, 'the reference iteration did not converge'
    return a


def logits_of(fs, fq, ys, ways, lam, alpha):
    """[nq, ways] logits of one task from the definition; differentiable in fs, fq, lam, alpha (tensors)."""
    g = fs @ fs.t()
    y = F.one_hot(ys.long(), ways).to(fs.dtype)
    a = solve_dual(g.detach(), ys.long(), ways, float(lam.detach()) if torch.is_tensor(lam) else float(lam)).to(fs.dtype)
    for _ in range(2):                                    # the implicit function theorem, by autograd through Newton steps at the optimum
        a = _newton_step(g, a, y, lam)
    return alpha * ((fq @ fs.t()) @ a)


def _leaves(fs, fq, ys, yq, lam, alpha, dtype):
    fs = torch.as_tensor(np.asarray(fs)).to(dtype).clone().requires_grad_(True)
    fq = torch.as_tensor(np.asarray(fq)).to(dtype).clone().requires_grad_(True)
    ys, yq = torch.as_tensor(np.asarray(ys)).long(), torch.as_tensor(np.asarray(yq)).long()
    T = fs.shape[0]
    lams = torch.full((T,), float(np.float32(lam)), dtype=dtype, requires_grad=True)
    alphas = torch.full((T,), float(np.float32(alpha)), dtype=dtype, requires_grad=True)
    return fs, fq, ys, yq, lams, alphas


_HEAD_CACHE = {}


def head(fs, fq, ys, yq, ways, lam, alpha, dtype=torch.float64):
    """fs [T, ns, F], fq [T, nq, F], ys [T, ns], yq [T, nq] (arrays or tensors).  Returns numpy (loss [T], acc [T], logits [T, nq, ways],
    dfs, dfq, dhyper [T, 2] = (dloss_t/dlam, dloss_t/dalpha)) with dfs, dfq the gradient of sum_t loss_t.  One run per input, kept and
    never modified."""
    key = (M.__name__, np.asarray(fs).tobytes(), np.asarray(fq).tobytes(), np.asarray(ys).tobytes(), np.asarray(yq).tobytes(), ways,
           float(lam), float(alpha), str(dtype))
    if key in _HEAD_CACHE:
        return _HEAD_CACHE[key]
    fs, fq, ys, yq, lams, alphas = _leaves(fs, fq, ys, yq, lam, alpha, dtype)
    losses, accs, logits = [], [], []
    for t in range(fs.shape[0]):
        z = logits_of(fs[t], fq[t], ys[t], ways, lams[t], alphas[t])
        losses.append(F.cross_entropy(z, yq[t]))
        accs.append(float(R.accuracy(z, yq[t])))
        logits.append(z.detach())
    torch.stack(losses).sum().backward()
    res = (torch.stack(losses).detach().double().numpy(), np.asarray(accs), torch.stack(logits).double().numpy(),
           fs.grad.double().numpy(), fq.grad.double().numpy(), torch.stack([lams.grad, alphas.grad], dim=1).double().numpy())
    for r in res:
        r.setflags(write=False)
    _HEAD_CACHE[key] = res
    return res


# ------------------------------------------------------------------------------------------- reference 2: the kernel's formulas and solver
def _c(u, p, v):
    """C V, row-wise: C_i = diag(u_i) (I - u_i u_i^T), u = sqrt(p); D_i = C_i C_i^T."""
    return u * v - p * (u * v).sum(axis=1, keepdims=True)


def _ct(u, p, v):
    return u * (v - (p * v).sum(axis=1, keepdims=True))


def _evaluate(g, a, hit, lam):
    """(P, U, R, |R|_inf, inner objective) at A; NaN anywhere gives NaN in both scalars."""
    s = g @ a
    mx = s.max(axis=1, keepdims=True)
    ex = np.exp(s - mx)
    se = ex.sum(axis=1, keepdims=True)
    p = ex / se
    r = lam * a + p - hit
    f = ((mx + np.log(se))[:, 0] - s[hit.astype(bool)]).sum() + 0.5 * lam * (a * s).sum()
    rn = np.abs(r).max() if np.isfinite(r).all() else np.nan
    return p, np.sqrt(p), r, float(rn), float(f)


def _apply_inverse(g, lam, p, u, v, cg_cap, count):
    """(lam I + D G)^-1 V = (V - C (lam I + C^T G C)^-1 C^T G V) / lam, the inner system (symmetric positive definite, eigenvalues >= lam)
    by conjugate gradients from 0 until |r|^2 <= CG_TOL^2 |b|^2.  Returns (result, converged); count[0] is raised to this solve's steps, count[1] grows by them."""
    b = _ct(u, p, g @ v)
    bb = float((b * b).sum())
    x, r, d, rr, steps = np.zeros_like(b), b.copy(), b.copy(), bb, 0
    while steps < cg_cap and rr > CG_TOL * CG_TOL * bb:
        q = lam * d + _ct(u, p, g @ _c(u, p, d))
        al = rr / float((d * q).sum())
        x = x + al * d
        r = r - al * q
        rn = float((r * r).sum())
        d = r + (rn / rr) * d
        rr = rn
        steps += 1
    count[0] = max(count[0], steps)
    count[1] += steps
    return (v - _c(u, p, x)) / lam, bool(rr <= CG_TOL * CG_TOL * bb)


def closed_form(fs, fq, ys, yq, ways, lam, alpha, round_out=False, gram_dtype=None, stop=STOP, accept=ACCEPT, cap=None):
    """The kernel's formulas and solver in fp64 NumPy; lam and alpha are the fp32 values the C entry receives.  Returns ``head``'s tuple and
    a dict of counts: newton (steps taken, the most over tasks), cg (the most steps of one solve), cg_total (the most CG steps of one task, its
    backward solve included), halve (the most halvings of one Newton step),
    residual (the largest final |R|_inf), flagged (tasks whose outputs the kernel would make NaN).
    round_out: loss, logits, dfs, dfq and dhyper are rounded to fp32 as a store does (the kernel has no fp32 intermediate: that is all of
    its model).  gram_dtype = np.float32: Fs Fs^T accumulated in fp32 (the first mutant).  stop = accept = 1e-5: a solver satisfied with a
    residual of 1e-5 (the second mutant)."""
    cap = cap or caps()
    fs, fq = np.asarray(fs, dtype=np.float32), np.asarray(fq, dtype=np.float32)
    ys, yq = np.asarray(ys), np.asarray(yq)
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    T, ns, _ = fs.shape
    nq = fq.shape[1]
    out = [[], [], [], [], [], []]
    info = dict(newton=0, cg=0, cg_total=0, halve=0, residual=0.0, flagged=0)
    cg = [0, 0]
    for t in range(T):
        s, q = fs[t].astype(np.float64), fq[t].astype(np.float64)
        g, k = s @ s.T, q @ s.T
        cg[1] = 0
        if gram_dtype is not None:
            g = (fs[t].astype(gram_dtype) @ fs[t].astype(gram_dtype).T).astype(np.float64)
        hit_s = (ys[t][:, None] == np.arange(ways)[None, :]).astype(np.float64)
        hit_q = yq[t][:, None] == np.arange(ways)[None, :]
        with np.errstate(all='ignore'):
            a = np.zeros((ns, ways))
            p, u, r, rn, f = _evaluate(g, a, hit_s, lam)
            newton = 0
            while newton < cap['newton'] and rn > stop:
                step_dir = -_apply_inverse(g, lam, p, u, r, cap['cg'], cg)[0]
                slope = float((r * (g @ step_dir)).sum())
                step, halvings, moved = 1.0, 0, False
                while True:
                    cand = a + step * step_dir
                    pt, ut, rt, rnt, ft = _evaluate(g, cand, hit_s, lam)
                    if not (np.isfinite(rnt) and np.isfinite(ft)):
                        rn = np.nan
                        break
                    if rnt < rn or (rn > accept and ft <= f + ARMIJO * step * slope):
                        a, p, u, r, rn, f, moved = cand, pt, ut, rt, rnt, ft, True
                        break
                    if rn <= accept or halvings == cap['halve']:
                        break
                    step *= 0.5
                    halvings += 1
                info['halve'] = max(info['halve'], halvings)
                if not moved:
                    break
                newton += 1
            bad = not rn <= accept
            info['newton'] = max(info['newton'], newton)
            info['residual'] = max(info['residual'], rn) if np.isfinite(rn) else np.nan
            pq = k @ a
            z = alpha * pq
            z32 = z.astype(np.float32)
            mx = z.max(axis=-1, keepdims=True)
            ex = np.exp(z - mx)
            se = ex.sum(axis=-1, keepdims=True)
            loss = ((mx + np.log(se))[:, 0] - z[hit_q]).sum() / nq
            acc = (z32.argmax(axis=-1) == yq[t]).mean()
            dz = (ex / se - hit_q.astype(np.float64)) / nq
            dalpha = (dz * pq).sum()
            dp = alpha * dz
            da = k.T @ dp
            x, conv = _apply_inverse(g, lam, p, u, p * da - p * (p * da).sum(axis=1, keepdims=True), cap['cg'], cg)
            bad = bad or not conv
            b = (da - g @ x) / lam
            dlam = -(b * a).sum()
            sm = -(x @ a.T + a @ x.T)
            dk = dp @ a.T
            res = [loss, acc, z, dk.T @ q + sm @ s, dk @ s, np.array([dlam, dalpha])]
        if bad:
            info['flagged'] += 1
            res = [np.full_like(np.asarray(v, dtype=np.float64), np.nan) for v in res]
        info['cg_total'] = max(info['cg_total'], cg[1])
        for o, v in zip(out, res):
            o.append(v)
    info['cg'] = cg[0]
    res = tuple(np.asarray(o, dtype=np.float64) for o in out)
    if round_out:
        res = tuple(r if i == 1 else r.astype(np.float32).astype(np.float64) for i, r in enumerate(res))
    return res + (info,)


# ---- the bar; every term comes from the references, none from the code under test
QUANTITIES = ('loss', 'logits', 'dfs', 'dfq', 'dlam', 'dalpha')
ROWWISE = ('logits', 'dfs', 'dfq')              # held per row as well: rows of nq, ns, nq
ULP32 = 2.0 ** -23


def quantities(o):
    """{name: array} of a (loss, acc, logits, dfs, dfq, dhyper, ...) tuple."""
    return dict(loss=o[0], logits=o[2], dfs=o[3], dfq=o[4], dlam=o[5][:, 0], dalpha=o[5][:, 1])


def rel(a, b, rows=False):
    """|a - b| / |b| in norm, over everything or per row of the last axis; a zero reference divides by 1e-300."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if rows:
        a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        return np.sqrt(((a - b) ** 2).sum(axis=-1)) / np.maximum(np.sqrt((b ** 2).sum(axis=-1)), 1e-300)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-300))


def bar_errors(got, o_head, o_cf):
    """{name: (error, bar)} for QUANTITIES and {name + '_rows': (errors, bars)} for ROWWISE.  The error is relative in norm against ``head``;
    the bar is 2^-23 + 2 e_dp + 2 e_ref: one fp32 ulp (the store's rounding takes half; device exp / log and the order of the fp64 sums the
    rest), e_dp = 0 (the kernel keeps no intermediate in fp32), e_ref = rel(closed_form, head), the two references' own disagreement."""
    got, o_head, o_cf = quantities(got), quantities(o_head), quantities(o_cf)
    res = {}
    for n in QUANTITIES:
        for rows in ((False, True) if n in ROWWISE else (False,)):
            res[n + '_rows' if rows else n] = (rel(got[n], o_head[n], rows), ULP32 + 2 * rel(o_cf[n], o_head[n], rows))
    return res


def flag_inputs():
    """(fs, fq, ys, yq) of the (feat 4, ways 2, ns 2, nq 2) case at T = 3 with a NaN planted in one element of task 1's fs."""
    fs, fq, ys, yq = kernel_inputs(4, 2, 2, 2, 3)
    fs[1, 1, 2] = np.nan
    return fs, fq, ys, yq


def meta_batch(theta_feat, base, fc, datas, labelss, shots, ways, lam, alpha, dtype=torch.float64):
    """The fused call: per task features = conv_base(data).view(-1, fc) on all 2n rows, prepare_batch's split, the logistic-regression head
    on (support, query), the sum of the tasks' losses backward into the trunk.  Returns a dict of numpy arrays: losses [T], accs [T], logits
    [T, n, ways], grad_feat (flat, parameters() order), dhyper [T, 2].  dtype float32: the trunk and the head's autograd in fp32 around the
    fp64 inner solve (an inner solve in fp32 cannot reach the residual the definition asks for)."""
    fl = OrderedDict((k, v.detach().to(dtype).clone().requires_grad_(True)) for k, v in theta_feat.items())
    leaves = list(fl.values())
    feats = lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc)
    T = len(datas)
    lams = torch.full((T,), float(lam), dtype=dtype, requires_grad=True)
    alphas = torch.full((T,), float(alpha), dtype=dtype, requires_grad=True)
    losses, accs, logits = [], [], []
    for t, (data, labels) in enumerate(zip(datas, labelss)):
        fs, ys, fq, yq = R.prepare_batch(data.to(dtype), labels, shots, ways, feats)
        g = fs @ fs.t()
        y = F.one_hot(ys.long(), ways).to(dtype)
        a = solve_dual(g.detach().double(), ys.long(), ways, float(lam)).to(dtype)
        for _ in range(2):
            a = _newton_step(g, a, y, lams[t])
        z = alphas[t] * ((fq @ fs.t()) @ a)
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
