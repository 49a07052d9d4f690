"""Cases, seeded inputs and fp64 references (TEST INFRASTRUCTURE) of the step-wise policy learner: mi_policy_vjp / mi_policy_hvp
(csrc/policy_learner.hip) against plain autograd on tests/policy_shapes_oracle.Oracle.

Cases: the eight of policy_shapes_oracle.CASES (their query batch; wide_160x132 lies outside the fused range and takes the per-layer
path) and the ones below, chosen by what the fused sweep does with them -- slabs of 16 rows (VJP) / 8 rows (HVP), at most 64
workgroups per task, 128-float LDS rows, one thread per column and half a slab of rows.

With s_t = sum over a task's valid rows of loc . dloc:  grad = ds_t/dtheta,  hv = (d^2 s_t / dtheta^2) v,  loc_dot = J v."""
import functools
import math
from collections import OrderedDict

import torch

import policy_shapes_oracle as PO
from oracle import rl_ref as RL

# name -> (S, A, H1, H2, activation, T, B, count, first seed of the search)
EXTRA = OrderedDict([
    # the DiagNormalPolicy defaults, both activations, and the Meta-World size: 33 rows = two VJP slabs + 1 (four HVP slabs + 1), the second
    # task ends inside a slab
    ('default_relu', (2, 2, 100, 100, 'relu', 2, 33, (33, 17), 100)),
    ('default_tanh', (2, 2, 100, 100, 'tanh', 2, 33, (33, 17), 200)),
    ('metaworld_relu', (9, 4, 100, 100, 'relu', 2, 33, (33, 17), 300)),
    # the fused predicate's upper limits: every LDS row and every accumulator block in use, tanh curvature in column 127
    ('limits_128', (16, 6, 128, 128, 'tanh', 2, 33, (33, 9), 400)),
    # H2 = 65: one column past a lane boundary (and H1 = 40: the last W2 accumulator blocks are partial in both directions)
    ('h2_65', (3, 2, 40, 65, 'relu', 2, 19, (19, 9), 500)),
    # more slabs than workgroups: 66 VJP / 131 HVP slabs on 64 workgroups, so a workgroup accumulates over several slabs; the rows
    # 1000 .. 1040 are padding: HVP slabs that are skipped whole
    ('loop_1041', (3, 2, 5, 3, 'tanh', 1, 1041, (1000,), 600)),
])
# the seeds the tests use: what find_seed returns (tests/test_policy_learner_host.py holds them to it)
SEEDS = dict(default_relu=100, default_tanh=200, metaworld_relu=300, limits_128=400, h2_65=500, loop_1041=600)

NAMES = list(PO.CASES) + list(EXTRA)
LR = PO.INNER_LR


def shape(name):
    """(S, A, H1, H2, activation, T, B) of a case."""
    return (PO.CASES[name] if name in PO.CASES else EXTRA[name])[:7]


def make_inputs(name, seed=None):
    """theta [P]; a batch (states, actions, adv, count; padding rows zero); cotangents dloc [T, B, A] and directions v [T, P]: seeded
    normals, exact in fp32.  The batch of a policy_shapes_oracle case is its query batch and the per-task parameters are the ones adapted
    on its first support batch -- the points policy_shapes_oracle.visit evaluates that batch at, so its margins hold here; the other
    cases adapt on the batch itself."""
    S, A, H1, H2, act, T, B = shape(name)
    if name in PO.CASES:
        inp = PO.make_inputs(name)
        theta, batch = inp['theta'], {k: inp['qry'][k] for k in ('states', 'actions', 'adv', 'count')}
        adapt_batch = PO.sup_k(inp, 0)
        g = torch.Generator().manual_seed(9000 + NAMES.index(name))
    else:
        g = torch.Generator().manual_seed(SEEDS[name] if seed is None else seed)
        rnd = lambda *shp: torch.randn(*shp, generator=g, dtype=torch.float64)
        parts = []
        for k, shp in RL.policy_param_shapes(S, A, (H1, H2)).items():
            if k == 'sigma':
                parts.append(torch.linspace(-0.4, 0.3, A, dtype=torch.float64))
            elif k.endswith('weight'):
                parts.append((rnd(*shp) / math.sqrt(shp[1])).reshape(-1))
            else:
                parts.append(0.1 * rnd(*shp))
        theta = PO._f32(torch.cat(parts))
        count = torch.tensor(EXTRA[name][7], dtype=torch.int32)
        batch = dict(states=PO._f32(rnd(T, B, S)), actions=PO._f32(rnd(T, B, A)), adv=PO._f32(rnd(T, B)), count=count)
        for t in range(T):
            for k in ('states', 'actions', 'adv'):
                batch[k][t, int(count[t]):] = 0.0
        adapt_batch = batch
    rnd = lambda *shp: PO._f32(torch.randn(*shp, generator=g, dtype=torch.float64))
    return dict(name=name, S=S, A=A, H=(H1, H2), activation=act, T=T, B=B, theta=theta, batch=batch, adapt_batch=adapt_batch, dloc=rnd(T, B, A),
                v=rnd(T, theta.numel()))


def products(o, inp, theta, head_only):
    """fp64 autograd: (grad [T, P], hv [T, P], loc_dot [T, B, A]) at theta [P] or [T, P]; rows past count are zero in loc_dot."""
    T, B, A = inp['T'], inp['B'], inp['A']
    grads, hvs, loc_dot = [], [], torch.zeros(T, B, A, dtype=torch.float64)
    for t in range(T):
        n = int(inp['batch']['count'][t])
        p = o.unflat(theta if theta.dim() == 1 else theta[t], leaf=True)
        plist = list(p.values())
        d = inp['dloc'][t, :n].double().clone().requires_grad_(True)
        loc = o.loc_scale(RL._body_detached(p, head_only), inp['batch']['states'][t, :n].double())[0]
        g = torch.autograd.grad((loc * d).sum(), plist, create_graph=True, allow_unused=True)
        g = torch.cat([(torch.zeros_like(q) if gi is None else gi).reshape(-1) for q, gi in zip(plist, g)])
        h = torch.autograd.grad((g * inp['v'][t].double()).sum(), plist + [d], allow_unused=True)
        grads.append(g.detach())
        hvs.append(torch.cat([(torch.zeros_like(q) if hi is None else hi).reshape(-1) for q, hi in zip(plist, h[:-1])]))
        loc_dot[t, :n] = h[-1]
    return torch.stack(grads), torch.stack(hvs), loc_dot


def visit(inp, with_products=True):
    """Everything tests/test_gpu_policy_learner.py compares -> (references, the oracle with its margin).  The parameter points: theta
    (shared) and one vector per task, the adapted parameters (exact in fp32)."""
    o = PO.Oracle(inp['S'], inp['A'], inp['H'], inp['activation'])
    ref = dict(theta_tasks=PO._f32(o.adapt(inp['theta'], inp['adapt_batch'], lr=LR)[0]))
    for per_task in (False, True):
        theta = ref['theta_tasks'] if per_task else inp['theta']
        if with_products:
            for head_only in (False, True):
                ref[per_task, head_only] = products(o, inp, theta, head_only)
        else:
            o.loc(theta, inp['batch']['states'], inp['batch']['count'])
    return ref, o


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, fp64 references, margin) of a case at its fixed seed: computed once, shared between the tests, read-only."""
    inp = make_inputs(name)
    ref, o = visit(inp)
    return inp, ref, o.margin


def find_seed(name):
    """As policy_shapes_oracle.find_seed, for the cases of EXTRA: the first of MAX_SEEDS seeds whose inputs keep every ReLU
    pre-activation MARGIN away from the kink at every parameter point -> (seed, margin)."""
    base = EXTRA[name][8]
    if EXTRA[name][4] != 'relu':
        return base, math.inf
    best = 0.0
    for seed in range(base, base + PO.MAX_SEEDS):
        m = visit(make_inputs(name, seed), with_products=False)[1].margin
        if m >= PO.MARGIN:
            return seed, m
        best = max(best, m)
    return None, best


class AutogradEngine:
    """Test double of PolicyEngine's ``forward`` / ``vjp`` / ``hvp`` on plain autograd, in the dtype of theta (the CPU tests run the
    policy in fp64): what the HIP entries compute, stated with the oracle's leaves."""

    def __init__(self, S, A, H, activation):
        self.act = torch.tanh if activation == 'tanh' else torch.relu
        self.shapes = RL.policy_param_shapes(S, A, H)
        self.calls = []

    def _loc(self, theta, states, head_only=False):
        p, off = OrderedDict(), 0
        for k, shp in self.shapes.items():
            n = int(math.prod(shp))
            p[k] = theta[off:off + n].reshape(shp)
            off += n
        return RL.policy_loc_scale(RL._body_detached(p, head_only), states.to(theta.dtype), self.act)[0]

    def _rows(self, theta, states, count, t):
        return (theta if theta.dim() == 1 else theta[t]), states[t, :states.shape[1] if count is None else int(count[t])]

    def forward(self, theta, states):
        self.calls.append('forward')
        with torch.no_grad():
            return torch.stack([self._loc(*self._rows(theta, states, None, t)) for t in range(states.shape[0])])

    @torch.enable_grad()
    def _products(self, theta, states, dloc, v, count, head_only):
        grads, hvs, loc_dot = [], [], torch.zeros(dloc.shape, dtype=theta.dtype)
        for t in range(states.shape[0]):
            th, x = self._rows(theta, states, count, t)
            th = th.detach().clone().requires_grad_(True)
            d = dloc[t, :x.shape[0]].detach().to(th.dtype).clone().requires_grad_(True)
            (g,) = torch.autograd.grad((self._loc(th, x, head_only) * d).sum(), th, create_graph=v is not None)
            grads.append(g.detach())
            if v is not None:
                h = torch.autograd.grad((g * v[t].to(th.dtype)).sum(), [th, d], allow_unused=True)
                hvs.append(torch.zeros_like(th) if h[0] is None else h[0])
                loc_dot[t, :x.shape[0]] = h[1]
        return torch.stack(grads), (torch.stack(hvs) if hvs else None), loc_dot

    def vjp(self, theta, states, dloc, count=None, head_only=False):
        self.calls.append('vjp')
        return self._products(theta, states, dloc, None, count, head_only)[0]

    def hvp(self, theta, states, dloc, v, count=None, head_only=False):
        self.calls.append('hvp')
        return self._products(theta, states, dloc, v, count, head_only)[1:]


def rows(batch, t):
    """(states, actions, adv [n, 1]) of a task's valid rows."""
    n = int(batch['count'][t])
    return batch['states'][t, :n], batch['actions'][t, :n], batch['adv'][t, :n].reshape(n, 1)


def plain_chain(inp, sups, qry, t, lr, first_order, head_only):
    """learn2learn's chain for task t in plain fp64 autograd: one update per support batch (first order: the gradients are constants;
    head_only: the body is a constant in the updates), the a2c loss on the query rows -> (theta_K [P], loss, its gradient at theta [P])."""
    act = torch.tanh if inp['activation'] == 'tanh' else torch.relu
    p0, off = OrderedDict(), 0
    for k, shp in RL.policy_param_shapes(inp['S'], inp['A'], inp['H']).items():
        n = int(math.prod(shp))
        p0[k] = inp['theta'][off:off + n].reshape(shp).clone().requires_grad_(True)
        off += n
    p = p0
    for sup in sups:
        s, a, adv = rows(sup, t)
        loss = -(RL.policy_log_prob(RL._body_detached(p, head_only), s, a, act) * adv).mean()
        g = torch.autograd.grad(loss, list(p.values()), create_graph=not first_order, allow_unused=True)
        p = OrderedDict((k, v if gk is None else v - lr * gk) for (k, v), gk in zip(p.items(), g))
    s, a, adv = rows(qry, t)
    loss = -(RL.policy_log_prob(p, s, a, act) * adv).mean()
    grad = torch.autograd.grad(loss, list(p0.values()), allow_unused=True)
    flat = lambda xs, like: torch.cat([(torch.zeros_like(q) if x is None else x).reshape(-1) for x, q in zip(xs, like)])
    return flat(list(p.values()), list(p.values())).detach(), loss.detach(), flat(grad, list(p0.values()))
