"""Oracle (TEST INFRASTRUCTURE) of the policy path on PADDED batches and at any widths: what PolicyEngine computes from
states [T,B,S], actions [T,B,A], adv [T,B], count [T] (and done [T,B] for the DiCE loss), restated with the leaves of oracle/rl_ref.py and
plain autograd (double backward for the products).  CPU, fp64 by default; ``dtype=torch.float32`` runs the same arithmetic in fp32 (the
conditioning yardstick of tests/test_gpu_policy_shapes.py).  Every network evaluation runs on a task's valid rows only and records the
smallest |pre-activation| it met (``Oracle.margin``): for a ReLU policy the fp32 engine takes the fp64 side of every kink only while that
margin is far above fp32 rounding.

Also here: the cases of tests/test_gpu_policy_shapes.py, their seeded inputs and the seed search (``find_seed``)."""
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from oracle import rl_ref as RL

MARGIN = 1e-5            # smallest |pre-activation| a ReLU case may meet at any parameter point the oracle visits
MAX_SEEDS = 32
DAMPING = 1e-5
INNER_LR = 0.1
CLIP = 0.1

# name -> (S, A, H1, H2, activation, T, B, count or None for ragged, first seed of the search).  What each case reaches in csrc/policy.hip --
# Kd is the reduction width of dense_mfma_kernel (forward: S, H1, H2; backward: H2, A, H1), I the input width of
# dense_wgrad_mfma_kernel (S, H1, H2).  (last_col_31x127 and k16_64x36 were first searched from 6000 and 7000: 32 and 18 seeds; the search
# starts closer to what it found so that the host test, which repeats it, stays short.)
CASES = OrderedDict([
    # Kd = 1 and 2 (scalar path); I + 1 = 2, 3: one tile; 5 and 3 rows: most of the 8 waves of the weight gradient get no row
    ('min_1x1', (2, 2, 1, 1, 'relu', 2, 5, (5, 3), 1002)),
    # Kd = 3, 5, 1 (scalar path), A = 1 and o_w1 = 1: every operand misaligned; I + 1 = 4, 6; a task with one valid row
    ('odd_5x3', (3, 1, 5, 3, 'tanh', 3, 33, (33, 20, 1), 2)),
    # Kd = 8, 12 (8-byte path, forward and backward); Kd = 50 (scalar path, 5 chunks of 10), Kd = 2; I + 1 = 9, 13, 51: two tiles; H1 < H2
    ('k8_12x50', (8, 2, 12, 50, 'relu', 3, 70, None, 3000)),
    # A = 6; Kd = 4 (8-byte), 33, 7, 6 (scalar); I + 1 = 34: the bias two columns into a second tile; H1 > H2
    ('a6_33x7', (4, 6, 33, 7, 'tanh', 2, 70, None, 4)),
    # Kd = 128 (16-byte, 32 chunks), Kd = 20 (16-byte, 5 chunks: odd against MI_DENSE_CU = 2); I = 128: a tile of the bias column alone
    ('bias_tile_128x20', (2, 2, 128, 20, 'tanh', 3, 70, None, 5)),
    # I + 1 = 32 and 128: the bias in a tile's last column; Kd = 31, 127 (scalar path, chunk tails of 1 and 7), Kd = 5
    ('last_col_31x127', (5, 2, 31, 127, 'relu', 3, 70, None, 6030)),
    # Kd = 16 in layer 1, 64 (% 8 == 0), 36 (% 8 == 4): 16-byte path; A = 4: 8-byte path with B not transposed; 129 rows: four slabs + 1
    ('k16_64x36', (16, 4, 64, 36, 'relu', 2, 129, None, 7010)),
    # O = 160, 132 > 128: five tile rows / columns; Kd = 160, 132 (16-byte); A = 3: odd o_w1
    ('wide_160x132', (2, 3, 160, 132, 'relu', 2, 40, None, 8000)),
])

# The seeds the tests use: what find_seed returns (tests/test_policy_shapes_host.py holds them to it and asserts the margins).
SEEDS = dict(min_1x1=1002, odd_5x3=2, k8_12x50=3008, a6_33x7=4, bias_tile_128x20=5, last_col_31x127=6031, k16_64x36=7017, wide_160x132=8009)

BLOCKS = ('sigma', 'W1', 'b1', 'W2', 'b2', 'W3', 'b3')


def block_slices(S, A, H1, H2):
    """The engine's flat parameter order (include/mi_maml.h): sigma, W1, b1, W2, b2, W3, b3."""
    out, off = OrderedDict(), 0
    for name, shp in zip(BLOCKS, RL.policy_param_shapes(S, A, (H1, H2)).values()):
        n = int(np.prod(shp))
        out[name] = slice(off, off + n)
        off += n
    return out


def _act(name):
    return torch.tanh if name == 'tanh' else torch.relu


class Oracle:
    def __init__(self, S, A, hiddens, activation='relu', dtype=torch.float64):
        self.S, self.A, self.H, self.activation, self.dtype = S, A, tuple(hiddens), activation, dtype
        self.shapes = RL.policy_param_shapes(S, A, self.H)
        self.names = list(self.shapes)
        self.P = sum(int(np.prod(s)) for s in self.shapes.values())
        self.margin = math.inf

    # ------------------------------------------------------------------------------------------- parameters
    def unflat(self, theta, leaf=False):
        theta = torch.as_tensor(theta).detach().to(self.dtype).reshape(-1)
        assert theta.numel() == self.P
        out, off = OrderedDict(), 0
        for k, shp in self.shapes.items():
            n = int(np.prod(shp))
            out[k] = theta[off:off + n].reshape(shp).clone().requires_grad_(leaf)
            off += n
        return out

    @staticmethod
    def flat(p):
        return torch.cat([v.reshape(-1) for v in p.values()])

    def _head(self, k):
        return k == 'sigma' or k.startswith('mean.4.')

    # ------------------------------------------------------------------------------------------- the network, valid rows only
    def _track(self, p, states):
        if self.activation != 'relu' or states.shape[0] == 0:
            return
        with torch.no_grad():
            h = states
            for i in (0, 2):
                z = torch.nn.functional.linear(h, p[f'mean.{i}.weight'], p[f'mean.{i}.bias'])
                self.margin = min(self.margin, float(z.abs().min()))
                h = torch.relu(z)

    def loc_scale(self, p, states):
        self._track(p, states)
        return RL.policy_loc_scale(p, states, _act(self.activation))

    def log_prob(self, p, states, actions):
        self._track(p, states)
        return RL.policy_log_prob(p, states, actions, _act(self.activation))

    def _rows(self, batch, t):
        n = int(batch['count'][t])
        c = lambda k, w: batch[k][t, :n].to(self.dtype).reshape(n, w)
        return dict(states=c('states', self.S), actions=c('actions', self.A), adv=c('adv', 1),
                    done=c('done', 1) if batch.get('done') is not None else None)

    def _loss(self, p, r, kind, old_lp=None, clip=CLIP, head_only=False):
        """a2c / dice: rl.py:208-228; ppo: rl.py:290 (old_lp None: against the policy itself, rl.py:312)."""
        lp = self.log_prob(RL._body_detached(p, head_only), r['states'], r['actions'])
        if kind == 'a2c':
            return RL.a2c_policy_loss(lp, r['adv'])
        if kind == 'dice':
            return RL.a2c_policy_loss(RL.dice_log_probs(lp, r['done']), r['adv'])
        assert kind == 'ppo'
        return RL.ppo_policy_loss(lp, lp.detach() if old_lp is None else old_lp, r['adv'], clip)

    def _step(self, p, loss, lr, head_only, second_order):
        """learn2learn maml_update: p - lr g for the parameters that received a gradient."""
        keep = [k for k in p if (not head_only) or self._head(k)]
        g = torch.autograd.grad(loss, [p[k] for k in keep], create_graph=second_order, retain_graph=second_order)
        new = OrderedDict(p)
        for k, gk in zip(keep, g):
            new[k] = p[k] - lr * gk
        return new

    # ------------------------------------------------------------------------------------------- quantities
    def loc(self, theta, states, count):
        """theta [P] or [T,P] -> loc [T,B,A] on the valid rows (zero elsewhere)."""
        T, B = states.shape[0], states.shape[1]
        theta = torch.as_tensor(theta)
        out = torch.zeros(T, B, self.A, dtype=self.dtype)
        for t in range(T):
            n = int(count[t])
            p = self.unflat(theta if theta.dim() == 1 else theta[t])
            out[t, :n] = self.loc_scale(p, states[t, :n].to(self.dtype))[0].detach()
        return out

    def adapt(self, theta, batch, lr=INNER_LR, head_only=False):
        """mi_policy_adapt: (theta_out [T,P], loss [T])."""
        T = batch['states'].shape[0]
        outs, losses = [], []
        for t in range(T):
            p = self.unflat(theta, leaf=True)
            loss = self._loss(p, self._rows(batch, t), 'a2c', head_only=head_only)
            outs.append(self.flat(self._step(p, loss, lr, head_only, False)).detach())
            losses.append(loss.detach())
        return torch.stack(outs), torch.stack(losses)

    def adapted_density(self, theta, sups, qry, lr=INNER_LR, head_only=False):
        """The stored old policies: K first-order updates from theta, then loc [T,B,A] (valid rows) and scale [T,A] on the query states."""
        T, B = qry['states'].shape[0], qry['states'].shape[1]
        loc, scale = torch.zeros(T, B, self.A, dtype=self.dtype), torch.zeros(T, self.A, dtype=self.dtype)
        for t in range(T):
            p = self.unflat(theta, leaf=True)
            for sup in sups:
                p = self._step(p, self._loss(p, self._rows(sup, t), 'a2c', head_only=head_only), lr, head_only, False)
                p = OrderedDict((k, v.detach().requires_grad_(True)) for k, v in p.items())
            n = int(qry['count'][t])
            l, s = self.loc_scale(p, qry['states'][t, :n].to(self.dtype))
            loc[t, :n], scale[t] = l.detach(), s.detach()
        return loc, scale

    def surrogate(self, theta, sups, qry, old_loc, old_scale, lr=INNER_LR, want_grad=True):
        """meta_surrogate_loss (rl.py:441-473) with K = len(sups) second-order updates -> dict(loss, kl, grad, kl_grad, hvp(v, damping)).
        hvp is trpo.hessian_vector_product of the mean KL: the Fisher-vector product where old equals the adapted policy, the exact
        Hessian-vector product otherwise."""
        T = qry['states'].shape[0]
        p0 = self.unflat(theta, leaf=True)
        loss, kl = 0.0, 0.0
        for t in range(T):
            p = OrderedDict((k, v.clone()) for k, v in p0.items())
            for sup in sups:
                p = self._step(p, self._loss(p, self._rows(sup, t), 'a2c'), lr, False, True)
            r = self._rows(qry, t)
            n = r['states'].shape[0]
            ol, os_ = old_loc[t, :n].to(self.dtype), old_scale[t].to(self.dtype)
            nl, ns = self.loc_scale(p, r['states'])
            kl = kl + RL.normal_kl(nl, ns, ol, os_).mean()
            old_lp = RL.normal_log_prob(ol, os_, r['actions']).mean(dim=1, keepdim=True)
            new_lp = RL.normal_log_prob(nl, ns, r['actions']).mean(dim=1, keepdim=True)
            loss = loss + RL.trpo_policy_loss(new_lp, old_lp, r['adv'])
        loss, kl = loss / T, kl / T
        out = dict(loss=loss.detach(), kl=kl.detach())
        if want_grad:
            plist = list(p0.values())
            out['grad'] = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, plist, retain_graph=True)]).detach()
            out['kl_grad'] = torch.cat([g.reshape(-1) for g in torch.autograd.grad(kl, plist, retain_graph=True)]).detach()
            out['hvp'] = lambda v, damping=DAMPING: RL.hessian_vector_product(kl, plist, damping)(v.to(self.dtype)).detach()
        return out

    def meta(self, theta, sup, qry, step_batch, lr=INNER_LR, kind='a2c', clip=CLIP, head_only=False, step_new_old=None):
        """mi_policy_meta_batch, second order: (loss [T], theta_out [T,P], grad [P] summed over tasks).  sup carries a leading batch axis."""
        T, K = qry['states'].shape[0], len(step_batch)
        if step_new_old is None:
            step_new_old = [1 if (k == 0 or step_batch[k] != step_batch[k - 1]) else 0 for k in range(K)]
        p0 = self.unflat(theta, leaf=True)
        losses, thetas, grad = [], [], torch.zeros(self.P, dtype=self.dtype)
        for t in range(T):
            p, old_lp = p0, None
            for k in range(K):
                r = self._rows({key: v[step_batch[k]] for key, v in sup.items() if v is not None}, t)
                if kind == 'ppo' and step_new_old[k]:
                    with torch.no_grad():
                        old_lp = self.log_prob(p, r['states'], r['actions'])
                p = self._step(p, self._loss(p, r, kind, old_lp, clip, head_only), lr, head_only, True)
            loss = self._loss(p, self._rows(qry, t), kind, None, clip)
            grad += torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, list(p0.values()))])
            losses.append(loss.detach())
            thetas.append(self.flat(p).detach())
        return torch.stack(losses), torch.stack(thetas), grad

    def update(self, theta, batch, lr=INNER_LR, kind='a2c', epochs=1, clip=CLIP):
        """mi_policy_update from shared parameters: (theta_out [T,P], loss [T,epochs])."""
        T = batch['states'].shape[0]
        outs, losses = [], torch.zeros(T, epochs, dtype=self.dtype)
        for t in range(T):
            p, r, old_lp = self.unflat(theta, leaf=True), self._rows(batch, t), None
            if kind == 'ppo':
                with torch.no_grad():
                    old_lp = self.log_prob(p, r['states'], r['actions'])
            for e in range(epochs):
                loss = self._loss(p, r, kind, old_lp, clip)
                losses[t, e] = loss.detach()
                p = OrderedDict((k, v.detach().requires_grad_(True)) for k, v in self._step(p, loss, lr, False, False).items())
            outs.append(self.flat(p).detach())
        return torch.stack(outs), losses


# --------------------------------------------------------------------------------------------------- inputs
def _f32(x):
    """fp64 values that fp32 holds exactly: the engine and the oracle start from the same numbers."""
    return x.float().double()


def make_inputs(name, seed=None):
    """Seeded inputs of a case: weights randn / sqrt(fan_in), biases 0.1 randn, sigma spread over [-0.4, 0.3]; two support batches and
    a query batch of randn states / actions / adv, padding rows zero; 'ragged': count[0] = B, the others in [B/2, B)."""
    S, A, H1, H2, act, T, B, count, _ = CASES[name]
    g = torch.Generator().manual_seed(SEEDS[name] if seed is None else seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    theta = OrderedDict()
    for k, shp in RL.policy_param_shapes(S, A, (H1, H2)).items():
        if k == 'sigma':
            theta[k] = torch.linspace(-0.4, 0.3, A, dtype=torch.float64) if A > 1 else torch.tensor([-0.4], dtype=torch.float64)
        elif k.endswith('weight'):
            theta[k] = rnd(*shp) / math.sqrt(shp[1])
        else:
            theta[k] = 0.1 * rnd(*shp)
    theta = _f32(torch.cat([v.reshape(-1) for v in theta.values()]))

    def batch():
        if count is None:
            c = torch.randint(B // 2, B, (T,), generator=g, dtype=torch.int32)
            c[0] = B
        else:
            c = torch.tensor(count, dtype=torch.int32)
        d = dict(states=_f32(rnd(T, B, S)), actions=_f32(rnd(T, B, A)), adv=_f32(rnd(T, B)),
                 done=(torch.rand(T, B, generator=g, dtype=torch.float64) < 0.15).double(), count=c)
        for t in range(T):
            n = int(c[t])
            d['done'][t, n - 1] = 1.0                              # a replay ends with the end of an episode
            for k in ('states', 'actions', 'adv', 'done'):
                d[k][t, n:] = 0.0
        return d
    b = [batch() for _ in range(3)]
    sup = {k: torch.stack([b[0][k], b[1][k]]) for k in b[0]}
    return dict(name=name, S=S, A=A, H=(H1, H2), activation=act, T=T, B=B, theta=theta, sup=sup, qry=b[2],
                cand=_f32(theta + 0.01 * torch.sin(torch.arange(theta.numel(), dtype=torch.float64))))


def sup_k(inp, k):
    return {key: v[k] for key, v in inp['sup'].items()}


def directions(inp, grad):
    """The two directions of every product: a seeded random one and the surrogate gradient normalised (both exact in fp32)."""
    g = torch.Generator().manual_seed(5)
    return [_f32(torch.randn(inp['theta'].numel(), generator=g, dtype=torch.float64)), _f32(grad / grad.norm())]


def visit(inp, dtype=torch.float64, products=True):
    """Every quantity tests/test_gpu_policy_shapes.py compares, in one walk -> (dict of references, the oracle with its margin).
    ``products=False`` leaves out gradients and double backward (the seed search: same network evaluations, a fraction of the time)."""
    o = Oracle(inp['S'], inp['A'], inp['H'], inp['activation'], dtype)
    th, qry, s0 = inp['theta'], inp['qry'], sup_k(inp, 0)
    sups = {1: [s0], 2: [s0, sup_k(inp, 1)]}
    ref = dict(loc=o.loc(th, qry['states'], qry['count']))
    for ho in (False, True):
        ref['adapt', ho] = o.adapt(th, s0, head_only=ho)
    ref['theta_tasks'] = _f32(ref['adapt', False][0])                  # per-task parameters for forward: the adapted ones
    ref['loc_tasks'] = o.loc(ref['theta_tasks'], qry['states'], qry['count'])
    for K in (1, 2):
        for case, ho in (('fisher', False), ('general', True)):
            old_loc, old_scale = (_f32(x) for x in o.adapted_density(th, sups[K], qry, head_only=ho))
            r = o.surrogate(th, sups[K], qry, old_loc, old_scale, want_grad=products)
            r['old_loc'], r['old_scale'] = old_loc, old_scale
            if products:
                r['v'] = directions(inp, r['grad'])
                r['hv'] = [r['hvp'](v) for v in r['v']]
                del r['hvp']
            c = o.surrogate(inp['cand'], sups[K], qry, old_loc, old_scale, want_grad=False)
            r['cand_loss'], r['cand_kl'] = c['loss'], c['kl']
            ref['trpo', K, case] = r
    for kind in ('a2c', 'ppo', 'dice'):
        for ho in ((False, True) if kind == 'a2c' else (False,)):
            ref['meta', kind, ho] = o.meta(th, inp['sup'], qry, [0, 1], kind=kind, head_only=ho)
    for kind in ('a2c', 'ppo'):
        ref['update', kind] = o.update(th, s0, kind=kind, epochs=2)
    return ref, o


@functools.lru_cache(maxsize=None)
def reference(name):
    """(inputs, fp64 references, margin) of a case at its fixed seed: computed once, shared between the tests, read-only."""
    inp = make_inputs(name)
    ref, o = visit(inp)
    return inp, ref, o.margin


def find_seed(name):
    """The first of MAX_SEEDS seeds from the case's base seed whose inputs keep every pre-activation the oracle meets MARGIN away from
    the ReLU kink -> (seed, margin); (None, best margin) if there is none.  tanh cases take their base seed."""
    base = CASES[name][8]
    if CASES[name][4] != 'relu':
        return base, math.inf
    best = 0.0
    for seed in range(base, base + MAX_SEEDS):
        m = visit(make_inputs(name, seed), products=False)[1].margin
        if m >= MARGIN:
            return seed, m
        best = max(best, m)
    return None, best
