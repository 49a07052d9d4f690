"""Oracle (TEST INFRASTRUCTURE) of the TRPO calls with per-parameter inner-loop step sizes: fp64 autograd over the leaves of
oracle/rl_ref.py (``policy_log_prob``, ``a2c_policy_loss``, ``trpo_policy_loss``, ``normal_kl``, ``compute_advantages``,
``collect_episodes``), which is imported and not edited.

``lr_vec [rows][P]`` is in the engine's order (sigma, W1, b1, W2, b2, W3, b3 -- the order of ``policy_param_shapes``); update k reads
row ``step_row[k]``; d_k is that row (times the head mask for the stored old policies of ANIL).

    theta_{k+1} = theta_k - d_k (.) g_k                      J_k = I - D_k H_k
    tangent  (J_k u):      u_{k+1} = u_k - d_k (.) (H_k u_k)
    adjoint  (J_k^T lam):  lam_k   = lam_{k+1} - H_k (d_k (.) lam_{k+1})
    surrogate gradient = mean_t lam_0,  lam_K = grad S_t(theta_K);     Fisher form (new == old) = mean_t J^T F_t J v + damping v
    exact KL Hessian:  rho_K = Hess KL_t(theta_K) u_K,
                       rho_k = rho_{k+1} - H_k (d_k (.) rho_{k+1}) - T_k[u_k, d_k (.) lam_{k+1}],     product = mean_t rho_0 + damping v

Two routes to the same numbers: ``autograd_route`` differentiates the whole surrogate / KL (double backward for the product);
``closed_form`` runs the recursions above with autograd only for g_k, H_k v, T_k[a, b] and the query derivatives.  ``closed_form`` also
offers the WRONG adjoint ``lam - d (.) (H lam)`` (what a scalar implementation turns into when its number becomes a vector): the tests
hold the right one apart from it.
"""
import functools
from collections import OrderedDict

import numpy as np
import torch

from oracle import rl_ref as RL

PARAMS = dict(inner_lr=0.1, max_path_length=25, adapt_steps=1, adapt_batch_size=6, meta_batch_size=4, outer_lr=0.3,
              backtrack_factor=0.5, ls_max_steps=15, max_kl=0.01, tau=1.0, gamma=0.99)
DAMPING = 1e-5
SPREAD = (0.25, 4.0)      # the per-entry factor of the GPU vector: base * U(0.25, 4) (tests/test_trpo_lr_host.py: why not U(0.5, 1.5))
FIELDS = ('states', 'actions', 'rewards', 'dones', 'next_states')


def _f32(x):
    return x.float().double()


class Net:
    """The policy as a flat fp64 vector in the engine's order."""

    def __init__(self, S=2, A=2, H=(100, 100), act='relu'):
        self.S, self.A, self.H, self.act_name = S, A, tuple(H), act
        self.act = torch.tanh if act == 'tanh' else torch.relu
        self.shapes = RL.policy_param_shapes(S, A, self.H)
        self.P = sum(int(np.prod(s)) for s in self.shapes.values())

    def unflat(self, v):
        out, off = OrderedDict(), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            out[k] = v[off:off + n].view(shp)
            off += n
        return out

    @staticmethod
    def flat(p):
        return torch.cat([v.reshape(-1) for v in p.values()])

    def mask(self, prefixes):
        m, off = torch.zeros(self.P, dtype=torch.bool), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            if any(k.startswith(pre) for pre in prefixes):
                m[off:off + n] = True
            off += n
        return m

    def head_mask(self):
        """1 on sigma and the last Linear (what the ANIL inner loop moves), 0 on the body."""
        last = max(int(k.split('.')[1]) for k in self.shapes if k.startswith('mean.'))
        return self.mask(('sigma', f'mean.{last}.')).double()

    def theta(self):
        from helpers import hash_params
        p = hash_params(self.shapes, 19)
        p['sigma'] = torch.tensor([-0.3, 0.2, -0.1, 0.1, 0.0, 0.25][:self.A], dtype=torch.float64)
        return _f32(self.flat(p))

    def baseline(self):
        return RL.LinearValue(self.S, self.A)          # the drivers pass env.action_size as the ridge coefficient


def lr_vector(net, base, rows, seed, frozen=('mean.0.',), spread=SPREAD, uniform=False):
    """[rows, P] step sizes exact in fp32: ``base`` * U(spread) per entry (``uniform``: ``base`` everywhere), the tensors whose names
    start with a ``frozen`` prefix at exactly 0."""
    g = torch.Generator().manual_seed(seed)
    lr = torch.full((rows, net.P), float(base), dtype=torch.float64)
    if not uniform:
        lr = lr * (spread[0] + (spread[1] - spread[0]) * torch.rand(rows, net.P, generator=g, dtype=torch.float64))
    lr = _f32(lr)
    lr[:, net.mask(frozen)] = 0.0
    return lr


def step_rows(rows, K):
    return [k if rows > 1 else 0 for k in range(K)]


# --------------------------------------------------------------------------------------------------- the pieces
def advantages(net, ep, params):
    """ch.normalize(compute_advantages(...)) with the baseline re-fitted to the replay (rl.py:95-110,355)."""
    return RL.normalize(RL.compute_advantages(net.baseline(), params['tau'], params['gamma'], ep)).detach()


def inner_loss(net, p, ep, adv):
    return RL.a2c_policy_loss(RL.policy_log_prob(p, ep['states'], ep['actions'], net.act), adv)


def update(net, th, ep, adv, d, head_only=False, create_graph=True):
    """theta - d (.) g on a flat vector.  head_only: the body is evaluated detached (DiagNormalPolicyANIL with features_no_grad), its
    gradient is None and the update leaves it alone whatever d holds there; the head's gradient does not depend on the detach, so
    this is d (.) head mask.  (First order only: the stored old policies.)"""
    (g,) = torch.autograd.grad(inner_loss(net, net.unflat(th), ep, adv), th, create_graph=create_graph)
    if not head_only:
        return th - d * g
    assert not create_graph
    return th - d * net.head_mask() * g


def query_terms(net, th, old, q, adv):
    """(surrogate loss, KL(new || old)) of one task at the adapted parameters th (rl.py:455-469)."""
    old_loc, old_scale = RL.policy_loc_scale(net.unflat(old), q['states'], net.act)
    old_loc, old_scale = old_loc.detach(), old_scale.detach()
    new_loc, new_scale = RL.policy_loc_scale(net.unflat(th), q['states'], net.act)
    kl = RL.normal_kl(new_loc, new_scale, old_loc, old_scale).mean()
    old_lp = RL.normal_log_prob(old_loc, old_scale, q['actions']).mean(dim=1, keepdim=True)
    new_lp = RL.normal_log_prob(new_loc, new_scale, q['actions']).mean(dim=1, keepdim=True)
    return RL.trpo_policy_loss(new_lp, old_lp, adv), kl


def adapt_plain(net, theta, task_replays, lr_vec, rows, params, head_only=False):
    """The stored old policy of a task: K first-order updates on its support replays (fast_adapt_trpo's loop on given replays)."""
    th = theta.detach()
    for k, ep in enumerate(task_replays[:-1]):
        th = update(net, th.clone().requires_grad_(True), ep, advantages(net, ep, params), lr_vec[rows[k]], head_only, False).detach()
    return th


# --------------------------------------------------------------------------------------------------- route 1: autograd through everything
def surrogate_graph(net, theta, replays, olds, lr_vec, rows, params):
    """(leaf theta, mean surrogate loss, mean KL) of rl.py:441-473 with the inner step p - lr_vec[rows[k]] (.) g, graph attached."""
    th0 = theta.detach().clone().requires_grad_(True)
    loss, kl = 0.0, 0.0
    for task, old in zip(replays, olds):
        th = th0
        for k, ep in enumerate(task[:-1]):
            th = update(net, th, ep, advantages(net, ep, params), lr_vec[rows[k]])
        s, c = query_terms(net, th, old, task[-1], advantages(net, task[-1], params))
        loss, kl = loss + s, kl + c
    return th0, loss / len(replays), kl / len(replays)


def meta_optimize(net, theta, replays, olds, lr_vec, rows, params, damping=DAMPING):
    """meta_optimize_trpo (rl.py:409-438) on that surrogate: conjugate gradient on the exact Hessian of the mean KL, the step scaled to
    max_kl, the backtracking line search.  -> dict(grad, step, accepted, theta (after the accepted step), fvp)."""
    th0, loss, kl = surrogate_graph(net, theta, replays, olds, lr_vec, rows, params)
    grad = torch.autograd.grad(loss, th0, retain_graph=True)[0].detach()
    (gkl,) = torch.autograd.grad(kl, th0, create_graph=True)
    fvp = lambda v: torch.autograd.grad(torch.dot(gkl, v), th0, retain_graph=True)[0].detach() + damping * v
    step = RL.conjugate_gradient(fvp, grad)
    step = step / torch.sqrt(0.5 * torch.dot(step, fvp(step)) / params['max_kl'])
    old_loss, accepted, new = float(loss.detach()), None, theta
    for ls in range(params['ls_max_steps']):
        cand = theta - params['backtrack_factor'] ** ls * params['outer_lr'] * step
        _, nl, nk = surrogate_graph(net, cand, replays, olds, lr_vec, rows, params)
        if float(nl.detach()) < old_loss and float(nk.detach()) < params['max_kl']:
            accepted, new = ls, cand.detach()
            break
    return dict(grad=grad, step=step, accepted=accepted, theta=new, fvp=fvp)


def autograd_route(net, theta, replays, olds, lr_vec, rows, params, vs=(), damping=DAMPING):
    """-> dict(loss, kl, grad, kl_grad, hvp [len(vs)]): the mean surrogate and mean KL of rl.py:441-473 with the inner step
    p - lr_vec[rows[k]] (.) g, their gradients, and the exact Hessian-vector products of the mean KL by double backward."""
    th0, loss, kl = surrogate_graph(net, theta, replays, olds, lr_vec, rows, params)
    (grad,) = torch.autograd.grad(loss, th0, retain_graph=True)
    (gkl,) = torch.autograd.grad(kl, th0, create_graph=True)
    hvp = [torch.autograd.grad(torch.dot(gkl, v), th0, retain_graph=True)[0].detach() + damping * v for v in vs]
    return dict(loss=float(loss.detach()), kl=float(kl.detach()), grad=grad.detach(), kl_grad=gkl.detach(), hvp=hvp)


# --------------------------------------------------------------------------------------------------- route 2: the recursions
def _zero_if_none(g, like):
    return torch.zeros_like(like) if g is None else g


def closed_form(net, theta, replays, olds, lr_vec, rows, params, vs=(), damping=DAMPING, wrong_order=False, tasks=None):
    """-> dict(grad, kl_grad, fisher [len(vs)], general [len(vs)], theta_K [T][P]) from the recursions of the module docstring.  Autograd
    forms g_k, H_k v, T_k[a, b] and the query derivatives only; every theta_k is a leaf.  ``wrong_order``: D H in place of H D on the
    adjoint side (and in the rho recursion), the implementation the tests must tell apart."""
    T = len(replays)
    acc = dict(grad=0.0, kl_grad=0.0, fisher=[0.0] * len(vs), general=[0.0] * len(vs))
    theta_K = []
    for task, old in zip(replays, olds):
        K = len(task) - 1
        ths, gs, th = [], [], theta.detach()
        for k in range(K):
            leaf = th.clone().requires_grad_(True)
            (g,) = torch.autograd.grad(inner_loss(net, net.unflat(leaf), task[k], advantages(net, task[k], params)), leaf, create_graph=True)
            ths.append(leaf); gs.append(g)
            th = (leaf - lr_vec[rows[k]] * g).detach()
        d = [lr_vec[rows[k]] for k in range(K)]
        theta_K.append(th)

        def H(k, v):
            return _zero_if_none(torch.autograd.grad(torch.dot(gs[k], v), ths[k], retain_graph=True, allow_unused=True)[0], v)

        def T3(k, a, b):                      # d/d eps H_k(theta_k + eps a) b
            (hb,) = torch.autograd.grad(torch.dot(gs[k], b), ths[k], create_graph=True)
            if not hb.requires_grad:
                return torch.zeros_like(a)
            return _zero_if_none(torch.autograd.grad(torch.dot(hb, a), ths[k], retain_graph=True, allow_unused=True)[0], a)

        leaf = th.clone().requires_grad_(True)
        s, c = query_terms(net, leaf, old, task[-1], advantages(net, task[-1], params))
        (gS,) = torch.autograd.grad(s, leaf, retain_graph=True)
        (gKL,) = torch.autograd.grad(c, leaf, create_graph=True)
        HKL = lambda u: torch.autograd.grad(torch.dot(gKL, u), leaf, retain_graph=True)[0]

        def adjoint(x, keep=None):
            for k in range(K - 1, -1, -1):
                if keep is not None:
                    keep[k + 1] = x
                x = x - (d[k] * H(k, x) if wrong_order else H(k, d[k] * x))
            return x

        def tangent(v):
            us = [v]
            for k in range(K):
                us.append(us[k] - d[k] * H(k, us[k]))
            return us

        lam = {}
        acc['grad'] = acc['grad'] + adjoint(gS.detach())
        acc['kl_grad'] = acc['kl_grad'] + adjoint(gKL.detach(), lam)
        for i, v in enumerate(vs):
            us = tangent(v)
            acc['fisher'][i] = acc['fisher'][i] + adjoint(HKL(us[K]))
            rho = HKL(us[K])
            for k in range(K - 1, -1, -1):
                if wrong_order:
                    rho = rho - d[k] * H(k, rho) - d[k] * T3(k, us[k], lam[k + 1])
                else:
                    rho = rho - H(k, d[k] * rho) - T3(k, us[k], d[k] * lam[k + 1])
            acc['general'][i] = acc['general'][i] + rho
    out = dict(grad=acc['grad'] / T, kl_grad=acc['kl_grad'] / T, theta_K=theta_K)
    out['fisher'] = [f / T + damping * v for f, v in zip(acc['fisher'], vs)]
    out['general'] = [g / T + damping * v for g, v in zip(acc['general'], vs)]
    return out


# --------------------------------------------------------------------------------------------------- cases
def synthetic_replay(net, episodes, length, gen):
    """A replay at any state / action widths (the Particles2D stand-in is 2-D): randn states and actions exact in fp32, rewards
    -|state|, an episode end every ``length`` rows."""
    n = episodes * length
    rnd = lambda *s: _f32(torch.randn(*s, generator=gen, dtype=torch.float64))
    states = rnd(n, net.S)
    dones = torch.zeros(n, 1, dtype=torch.float64)
    dones[length - 1::length] = 1.0
    return dict(states=states, actions=rnd(n, net.A), rewards=-states.norm(dim=1, keepdim=True), dones=dones, next_states=rnd(n, net.S))


def cut_last_episode(ep):
    ends = torch.nonzero(ep['dones'].reshape(-1)).reshape(-1)
    n = int(ends[-2]) + 1
    assert 0 < n < ep['states'].shape[0]
    return {k: v[:n].clone() for k, v in ep.items()}


# name -> (S, A, H, activation, K, lr rows, anil, base step, tasks, ragged).  The 2-100-100-2 cases are the small case of
# tests/test_gpu_rl.py (4 tasks, 6 episodes x <= 25 steps, Particles2D); 3-19-33-1 (P = 771: every block of the parameter vector
# misaligned, no width a multiple of a tile) runs on synthetic replays, tanh so that no ReLU kink decides between fp32 and fp64.
CASES = OrderedDict([
    ('relu_k1', (2, 2, (100, 100), 'relu', 1, 1, False, 0.1, 4, False)),
    ('relu_k2', (2, 2, (100, 100), 'relu', 2, 2, False, 0.05, 4, False)),
    ('relu_k3', (2, 2, (100, 100), 'relu', 3, 3, False, 0.05, 2, False)),
    ('tanh_k1', (2, 2, (100, 100), 'tanh', 1, 1, False, 0.1, 4, False)),
    ('anil_tanh_k1', (2, 2, (100, 100), 'tanh', 1, 1, True, 0.1, 4, False)),
    ('anil_relu_k1', (2, 2, (100, 100), 'relu', 1, 1, True, 0.1, 4, False)),
    ('anil_tanh_k2', (2, 2, (100, 100), 'tanh', 2, 2, True, 0.1, 4, False)),
    ('anil_relu_k2', (2, 2, (100, 100), 'relu', 2, 2, True, 0.1, 4, False)),
    ('anil_tanh_k2_ragged', (2, 2, (100, 100), 'tanh', 2, 2, True, 0.1, 4, True)),
    ('odd_t1', (3, 1, (19, 33), 'tanh', 2, 2, True, 0.1, 1, False)),
    ('odd_t3', (3, 1, (19, 33), 'tanh', 2, 2, True, 0.1, 3, False)),
])


@functools.lru_cache(maxsize=None)
def make_case(name, spread=SPREAD, uniform=False):
    """-> dict(net, params, theta [P], lr_vec [rows, P], rows [K], replays [task][K + 1], olds [task] flat, anil).  The replays come from
    the oracle's own fast-adapt walk under the step-size vector (the old policies are what that walk ends with: adapted with d, or under
    ``anil`` with d (.) head mask).  Computed once per case; read-only."""
    S, A, H, act, K, nrows, anil, base, T, ragged = CASES[name]
    net = Net(S, A, H, act)
    params = dict(PARAMS, adapt_steps=K, inner_lr=base, meta_batch_size=T)
    theta = net.theta()
    lr_vec = lr_vector(net, base, nrows, 7, spread=spread, uniform=uniform)
    rows = step_rows(nrows, K)
    gen = torch.Generator().manual_seed(2)
    env = RL.Particles2D(seed=1) if (S, A) == (2, 2) else None
    tasks = env.sample_tasks(T) if env else [None] * T
    replays, olds = [], []
    for task in tasks:
        if env:
            env.set_task(task)
        th, rep = theta, []
        for k in range(K + 1):
            if env:
                ep = RL.collect_episodes(env, net.unflat(th), params['adapt_batch_size'], params['max_path_length'], gen, activation=net.act)
            else:
                ep = synthetic_replay(net, 4, 11 + 2 * k, gen)
            rep.append(ep)
            if k < K:
                th = update(net, th.clone().requires_grad_(True), ep, advantages(net, ep, params), lr_vec[rows[k]], anil, False).detach()
        replays.append(rep)
    if ragged:               # task 1's second support replay and task 2's query replay lose their last episode
        replays[1][1] = cut_last_episode(replays[1][1])
        replays[2][K] = cut_last_episode(replays[2][K])
    # the stored old policies on the replays as they are now (a cut replay changes the walk's later steps)
    olds = [adapt_plain(net, theta, rep, lr_vec, rows, params, head_only=anil) for rep in replays]
    return dict(net=net, params=params, theta=theta, lr_vec=lr_vec, rows=rows, replays=replays, olds=olds, anil=anil, name=name)


def directions(net, kl_grad=None):
    """The seed-5 random direction and, where the KL gradient is not zero, g_KL / |g_KL| (tests/test_gpu_anil_trpo_steps.py)."""
    vs = [_f32(torch.randn(net.P, generator=torch.Generator().manual_seed(5), dtype=torch.float64))]
    if kl_grad is not None and float(kl_grad.norm()) > 0:
        vs.append(_f32(kl_grad / kl_grad.norm()))
    return vs


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 reference of a case: autograd_route with the two directions (the second only where new != old)."""
    c = make_case(name)
    first = autograd_route(c['net'], c['theta'], c['replays'], c['olds'], c['lr_vec'], c['rows'], c['params'])
    vs = directions(c['net'], first['kl_grad'] if c['anil'] else None)
    out = autograd_route(c['net'], c['theta'], c['replays'], c['olds'], c['lr_vec'], c['rows'], c['params'], vs)
    out['vs'] = vs
    return out


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
