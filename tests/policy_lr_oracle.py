"""Oracle (TEST INFRASTRUCTURE) of the policy's fused calls with per-parameter inner-loop step sizes (mi_policy_meta_batch_lr /
mi_policy_update_lr): plain autograd, fp64 by default and fp32 as the conditioning yardstick, over the leaves of
oracle/rl_ref.py (``policy_log_prob``, ``a2c_policy_loss`` / ``dice_log_probs`` / ``ppo_policy_loss`` -- the bodies of its ``vpg_a2c_loss`` and
``replay_ppo`` -- on replays from its ``collect_episodes`` with advantages from its ``compute_advantages``), with what the feature adds:
the update ``p[k] - lr[k] * g`` with one ``lr`` leaf per entry and row, the ``head_only`` detach, and PPO's epochs sharing their adapt step's
row.  ``Oracle.meta_lr`` returns the losses, the adapted parameters, the meta-gradient summed over tasks and ``lr_grad``.

``closed_form`` states the recursion of section 21 itself (autograd only for g_k, H_k v and the query gradient):
    theta_{k+1} = theta_k - d_k g_k,  d_k = lr[row(k)] m;   lam_K = grad L_query(theta_K);   lam_k = lam_{k+1} - m H_k (d_k lam_{k+1})
    (first order: lam_k = lam_K);   grad = sum_t lam_0;   lr_grad[r] = - sum_{k: row(k) = r} sum_t m g_k lam_{k+1}
tests/test_policy_lr_host.py holds it to the autograd form at 1e-12."""
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from oracle import rl_ref as RL
import policy_shapes_oracle as PS

CLIP = 0.1


class Oracle(PS.Oracle):
    """``policy_shapes_oracle.Oracle`` (padded batches, any widths, valid rows only) with the step-size-vector calls."""

    def head_mask(self):
        m, off = torch.zeros(self.P, dtype=self.dtype), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            if self._head(k):
                m[off:off + n] = 1.0
            off += n
        return m

    def _lr_views(self, lr_row):
        """One row [P] of the step sizes as per-parameter views (connected to the leaf)."""
        out, off = OrderedDict(), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            out[k] = lr_row[off:off + n].reshape(shp)
            off += n
        return out

    def _step_lr(self, p, loss, lr_row, head_only, second_order):
        """p[k] - lr[k] * g, elementwise, for the parameters that received a gradient (head_only: sigma and the last Linear)."""
        keep = [k for k in p if (not head_only) or self._head(k)]
        g = torch.autograd.grad(loss, [p[k] for k in keep], create_graph=second_order, retain_graph=second_order)
        lrs = self._lr_views(lr_row)
        new = OrderedDict(p)
        for k, gk in zip(keep, g):
            new[k] = p[k] - lrs[k] * gk
        return new

    def meta_lr(self, theta, sup, qry, step_batch, lr_vec, step_lr_row=None, kind='a2c', clip=CLIP, head_only=False, first_order=False,
                step_new_old=None):
        """mi_policy_meta_batch_lr: (loss [T], theta_out [T,P], grad [P] summed over tasks, lr_grad [rows,P]).  sup carries a leading
        batch axis; update k replays batch step_batch[k] with row step_lr_row[k] (None: row 0)."""
        T, K = qry['states'].shape[0], len(step_batch)
        if step_new_old is None:
            step_new_old = [1 if (k == 0 or step_batch[k] != step_batch[k - 1]) else 0 for k in range(K)]
        rows = [0] * K if step_lr_row is None else list(step_lr_row)
        lr = torch.as_tensor(lr_vec).detach().to(self.dtype).reshape(-1, self.P).clone().requires_grad_(True)
        p0 = self.unflat(theta, leaf=True)
        losses, thetas = [], []
        grad, lr_grad = torch.zeros(self.P, dtype=self.dtype), torch.zeros_like(lr)
        for t in range(T):
            p, old_lp = p0, None
            for k in range(K):
                r = self._rows({key: v[step_batch[k]] for key, v in sup.items() if v is not None}, t)
                if kind == 'ppo' and step_new_old[k]:
                    with torch.no_grad():
                        old_lp = self.log_prob(p, r['states'], r['actions'])
                p = self._step_lr(p, self._loss(p, r, kind, old_lp, clip, head_only), lr[rows[k]], head_only, not first_order)
            loss = self._loss(p, self._rows(qry, t), kind, None, clip)
            gs = torch.autograd.grad(loss, list(p0.values()) + [lr], allow_unused=True)
            grad += torch.cat([g.reshape(-1) for g in gs[:-1]])
            if gs[-1] is not None:
                lr_grad += gs[-1]
            losses.append(loss.detach())
            thetas.append(self.flat(p).detach())
        return torch.stack(losses), torch.stack(thetas), grad, lr_grad.detach()

    def update_lr(self, theta, batch, lr_row, kind='a2c', epochs=1, clip=CLIP, head_only=False):
        """mi_policy_update_lr from shared parameters: theta_out [T,P]."""
        T = batch['states'].shape[0]
        lr_row = torch.as_tensor(lr_row).detach().to(self.dtype).reshape(self.P)
        outs = []
        for t in range(T):
            p, r, old_lp = self.unflat(theta, leaf=True), self._rows(batch, t), None
            if kind == 'ppo':
                with torch.no_grad():
                    old_lp = self.log_prob(p, r['states'], r['actions'])
            for _ in range(epochs):
                new = self._step_lr(p, self._loss(p, r, kind, old_lp, clip, head_only), lr_row, head_only, False)
                p = OrderedDict((k, v.detach().requires_grad_(True)) for k, v in new.items())
            outs.append(self.flat(p).detach())
        return torch.stack(outs)


def closed_form(o, theta, sup, qry, step_batch, lr_vec, step_lr_row=None, kind='a2c', clip=CLIP, head_only=False, first_order=False,
                step_new_old=None):
    """The recursion of the module docstring -> (loss [T], theta_out [T,P], grad [P], lr_grad [rows,P])."""
    T, K = qry['states'].shape[0], len(step_batch)
    if step_new_old is None:
        step_new_old = [1 if (k == 0 or step_batch[k] != step_batch[k - 1]) else 0 for k in range(K)]
    rows = [0] * K if step_lr_row is None else list(step_lr_row)
    lr = torch.as_tensor(lr_vec).detach().to(o.dtype).reshape(-1, o.P)
    m = o.head_mask() if head_only else torch.ones(o.P, dtype=o.dtype)
    flat = lambda gs, ps: torch.cat([(torch.zeros_like(q) if g is None else g).reshape(-1) for g, q in zip(gs, ps)])
    losses, thetas = [], []
    grad, lr_grad = torch.zeros(o.P, dtype=o.dtype), torch.zeros_like(lr)
    for t in range(T):
        th, kept, old_lp = torch.as_tensor(theta).detach().to(o.dtype).reshape(-1), [], None
        for k in range(K):
            r = o._rows({key: v[step_batch[k]] for key, v in sup.items() if v is not None}, t)
            p = o.unflat(th, leaf=True)
            if kind == 'ppo' and step_new_old[k]:
                with torch.no_grad():
                    old_lp = o.log_prob(p, r['states'], r['actions'])
            pl = list(p.values())
            g = flat(torch.autograd.grad(o._loss(p, r, kind, old_lp, clip, head_only), pl, create_graph=True, allow_unused=True), pl)
            kept.append((g, pl))
            th = th - lr[rows[k]] * m * g.detach()
        pK = o.unflat(th, leaf=True)
        pl = list(pK.values())
        loss = o._loss(pK, o._rows(qry, t), kind, None, clip)
        lam = flat(torch.autograd.grad(loss, pl, allow_unused=True), pl)
        lamK = lam
        for k in reversed(range(K)):
            g, plk = kept[k]
            lr_grad[rows[k]] -= m * g.detach() * (lamK if first_order else lam)
            if not first_order and g.requires_grad:
                hv = flat(torch.autograd.grad(g, plk, grad_outputs=lr[rows[k]] * m * lam, allow_unused=True), plk)
                lam = lam - m * hv
        grad += lam
        losses.append(loss.detach())
        thetas.append(th)
    return torch.stack(losses), torch.stack(thetas), grad, lr_grad


# --------------------------------------------------------------------------------------------------- inputs
def _f32(x):
    return x.float().double()


def lr_vector(o, base, rows, seed, frozen=('mean.0.',), uniform=False):
    """[rows, P] step sizes exact in fp32: ``base`` * U(0.5, 1.5) per entry (``uniform``: ``base`` everywhere), the tensors whose names start
    with a ``frozen`` prefix at exactly 0."""
    g = torch.Generator().manual_seed(seed)
    lr = torch.full((rows, o.P), float(base), dtype=torch.float64)
    if not uniform:
        lr = lr * (0.5 + torch.rand(rows, o.P, generator=g, dtype=torch.float64))
    lr = _f32(lr)
    lr[:, frozen_mask(o, frozen)] = 0.0
    return lr


def frozen_mask(o, frozen=('mean.0.',)):
    m, off = torch.zeros(o.P, dtype=torch.bool), 0
    for k, shp in o.shapes.items():
        n = int(np.prod(shp))
        if any(k.startswith(pre) for pre in frozen):
            m[off:off + n] = True
        off += n
    return m


def random_inputs(S, A, H, T, B, counts, seed, n_sup=2):
    """Seeded padded batches at any widths, as ``policy_shapes_oracle.make_inputs`` draws them: weights randn / sqrt(fan_in), biases
    0.1 randn, sigma over [-0.4, 0.3]; randn states / actions / adv exact in fp32, rows past ``counts[b][t]`` zero, an episode end on the
    last valid row.  counts: [n_sup + 1][T]."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    theta = OrderedDict()
    for k, shp in RL.policy_param_shapes(S, A, tuple(H)).items():
        if k == 'sigma':
            theta[k] = torch.linspace(-0.4, 0.3, A, dtype=torch.float64) if A > 1 else torch.tensor([-0.4], dtype=torch.float64)
        elif k.endswith('weight'):
            theta[k] = rnd(*shp) / math.sqrt(shp[1])
        else:
            theta[k] = 0.1 * rnd(*shp)
    theta = _f32(torch.cat([v.reshape(-1) for v in theta.values()]))

    def batch(c):
        c = torch.tensor(c, dtype=torch.int32)
        d = dict(states=_f32(rnd(T, B, S)), actions=_f32(rnd(T, B, A)), adv=_f32(rnd(T, B)),
                 done=(torch.rand(T, B, generator=g, dtype=torch.float64) < 0.15).double(), count=c)
        for t in range(T):
            n = int(c[t])
            d['done'][t, n - 1] = 1.0
            for k in ('states', 'actions', 'adv', 'done'):
                d[k][t, n:] = 0.0
        return d
    b = [batch(c) for c in counts]
    sup = {k: torch.stack([x[k] for x in b[:n_sup]]) for k in b[0]}
    return dict(S=S, A=A, H=tuple(H), T=T, B=B, theta=theta, sup=sup, qry=b[n_sup])


@functools.lru_cache(maxsize=None)
def particle_replays(activation, algo, T=3, adapt_steps=2):
    """The replays of tests/test_gpu_rl.py::test_policy_meta_batch_vpg_ppo as padded fp64 batches: 2-100-100-2 policy (hash weights, seed
    19), Particles2D(seed=3), per task ``adapt_steps`` support replays of 5 episodes of 12 / 15 steps and a query replay of 5 x 15 from
    ``collect_episodes`` (generator seed 4), advantages from ``compute_advantages`` with a fresh LinearValue per replay (normalised for
    'ppo').  Computed once per (activation, algo); read-only."""
    from helpers import hash_params
    act = torch.relu if activation == 'relu' else torch.tanh
    theta = hash_params(RL.policy_param_shapes(), 19)
    theta['sigma'] = torch.tensor([-0.3, 0.2], dtype=torch.float64)
    env = RL.Particles2D(seed=3)
    gen = torch.Generator().manual_seed(4)
    sup, qry = [[None] * T for _ in range(adapt_steps)], [None] * T
    for t, task in enumerate(env.sample_tasks(T)):
        env.set_task(task)
        for b in range(adapt_steps):
            sup[b][t] = RL.collect_episodes(env, theta, 5, 12 + 3 * b, gen, activation=act)
        qry[t] = RL.collect_episodes(env, theta, 5, 15, gen, activation=act)

    def adv_of(ep):
        a = RL.compute_advantages(RL.LinearValue(2, 2), 1.0, 0.99, ep)
        return (RL.normalize(a) if algo == 'ppo' else a).detach()
    B = max(int(e['states'].shape[0]) for row in sup + [qry] for e in row)

    def pad(row):
        d = dict(states=torch.zeros(T, B, 2, dtype=torch.float64), actions=torch.zeros(T, B, 2, dtype=torch.float64),
                 adv=torch.zeros(T, B, dtype=torch.float64), done=torch.zeros(T, B, dtype=torch.float64),
                 count=torch.zeros(T, dtype=torch.int32))
        for t, e in enumerate(row):
            n = int(e['states'].shape[0])
            d['states'][t, :n], d['actions'][t, :n], d['count'][t] = e['states'], e['actions'], n
            d['adv'][t, :n], d['done'][t, :n] = adv_of(e).reshape(-1), e['dones'].reshape(-1)
        return {k: (_f32(v) if v.dtype == torch.float64 else v) for k, v in d.items()}       # what the fp32 engine is handed
    sups = [pad(r) for r in sup]
    flat = _f32(torch.cat([v.reshape(-1) for v in theta.values()]))
    return dict(S=2, A=2, H=(100, 100), T=T, B=B, theta=flat, sup={k: torch.stack([s[k] for s in sups]) for k in sups[0]}, qry=pad(qry))


def task_slice(inp, ts):
    """The inputs restricted to the tasks ``ts`` (a list)."""
    out = dict(inp, T=len(ts))
    out['sup'] = {k: v[:, ts] for k, v in inp['sup'].items()}
    out['qry'] = {k: v[ts] for k, v in inp['qry'].items()}
    return out
