"""tests/policy_shapes_oracle.py held to oracle/rl_ref.py where both apply (the 2-100-100-2 policy on the small golden cases of
tests/rl_cases.py, 1e-12 relative), and the inputs of tests/test_gpu_policy_shapes.py checked on the CPU: the seed search of every case
gives the seed the GPU tests use, every ReLU pre-activation the oracle meets stays 1e-5 away from the kink, and every reference block the
GPU tests divide by is nonzero."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import policy_shapes_oracle as PO
import rl_cases
from oracle import rl_ref as RL


def _rel(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).norm() / b.norm())


def _padded(eps, params):
    """One replay per task -> the padded batch the engine takes, advantages as trpo_a2c_loss / meta_surrogate_loss make them."""
    T, B = len(eps), max(int(e['states'].shape[0]) for e in eps)
    d = dict(states=torch.zeros(T, B, 2, dtype=torch.float64), actions=torch.zeros(T, B, 2, dtype=torch.float64),
             adv=torch.zeros(T, B, dtype=torch.float64), done=torch.zeros(T, B, dtype=torch.float64), count=torch.zeros(T, dtype=torch.int32))
    for t, e in enumerate(eps):
        n = int(e['states'].shape[0])
        adv = RL.normalize(RL.compute_advantages(RL.LinearValue(2, 2), params['tau'], params['gamma'], e)).detach()
        d['states'][t, :n], d['actions'][t, :n], d['adv'][t, :n], d['done'][t, :n], d['count'][t] = \
            e['states'], e['actions'], adv.reshape(-1), e['dones'].reshape(-1), n
    return d


@pytest.mark.parametrize('name', ['small_relu', 'anil_tanh', 'two_steps'])
def test_oracle_reproduces_rl_ref_at_the_default_widths(golden_rl, name):
    """meta_surrogate_loss, its gradient, the mean KL and its Hessian-vector product, and trpo_update: small_relu is the Fisher case
    (KL = 0 up to rounding), anil_tanh the general one (head-only old policies, tanh), two_steps runs K = 2."""
    case = rl_cases.load_case(golden_rl, name)
    params, act, anil = case['params'], case['activation'], case['anil']
    K = params['adapt_steps']
    o = PO.Oracle(2, 2, (100, 100), 'tanh' if act is torch.tanh else 'relu')
    theta = torch.cat([v.reshape(-1) for v in case['theta'].values()])
    sups = [_padded([task[k] for task in case['replays']], params) for k in range(K)]
    qry = _padded([task[K] for task in case['replays']], params)
    T, B = qry['states'].shape[0], qry['states'].shape[1]
    old_loc, old_scale = torch.zeros(T, B, 2, dtype=torch.float64), torch.zeros(T, 2, dtype=torch.float64)
    for t, old in enumerate(case['olds']):
        n = int(qry['count'][t])
        old_loc[t, :n], old_scale[t] = RL.policy_loc_scale(old, qry['states'][t, :n], act)
    got = o.surrogate(theta, sups, qry, old_loc, old_scale, lr=params['inner_lr'])

    p64 = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in case['theta'].items())
    loss, kl = RL.meta_surrogate_loss(case['replays'], case['olds'], p64, RL.LinearValue(2, 2), params, activation=act)
    plist = list(p64.values())
    grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, plist, retain_graph=True)])
    v = torch.randn(grad.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    hv = RL.hessian_vector_product(kl, plist, PO.DAMPING)(v)
    loss, kl = loss.detach(), kl.detach()
    # (the summands, ratio x normalised advantage, have unit variance and zero mean: where new == old the loss itself is rounding noise)
    assert abs(float(got['loss']) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert _rel(got['grad'], grad) <= 1e-12
    assert _rel(got['hvp'](v), hv) <= 1e-12
    if anil:
        assert float(kl) > 1e-6 and abs(float(got['kl']) - float(kl)) <= 1e-12 * float(kl)
    else:
        assert abs(float(got['kl']) - float(kl)) <= 1e-24                       # both are rounding noise around zero
    # trpo_update on every task's first support replay
    th_out, _ = o.adapt(theta, sups[0], lr=params['inner_lr'], head_only=anil)
    for t, task in enumerate(case['replays']):
        p = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in case['theta'].items())
        new = RL.trpo_update(task[0], p, RL.LinearValue(2, 2), params['inner_lr'], params['gamma'], params['tau'], first_order=True,
                             activation=act, head_only=anil)
        ref = torch.cat([x.detach().reshape(-1) for x in new.values()])
        assert _rel(th_out[t] - theta, ref - theta) <= 1e-12
        assert _rel(th_out[t], ref) <= 1e-14


def test_oracle_meta_and_update_reproduce_rl_ref_replays():
    """The K-update VPG / DiCE / PPO walk (RL.replay_vpg / replay_ppo semantics on given advantages) on one task of synthetic rows: the
    oracle's meta() and update() against a direct restatement with the rl_ref leaves."""
    inp = PO.make_inputs('odd_5x3')
    o = PO.Oracle(inp['S'], inp['A'], inp['H'], inp['activation'])
    for kind in ('a2c', 'dice', 'ppo'):
        loss, th, grad = o.meta(inp['theta'], inp['sup'], inp['qry'], [0, 1], kind=kind)
        p0 = o.unflat(inp['theta'], leaf=True)
        gsum = torch.zeros(o.P, dtype=torch.float64)
        for t in range(inp['T']):
            p = p0
            for b in (0, 1):
                n = int(inp['sup']['count'][b, t])
                s, a = inp['sup']['states'][b, t, :n], inp['sup']['actions'][b, t, :n]
                adv, dn = inp['sup']['adv'][b, t, :n].reshape(-1, 1), inp['sup']['done'][b, t, :n].reshape(-1, 1)
                lp = RL.policy_log_prob(p, s, a, torch.tanh)
                if kind == 'ppo':
                    l = RL.ppo_policy_loss(lp, lp.detach(), adv, PO.CLIP)
                else:
                    l = RL.a2c_policy_loss(RL.dice_log_probs(lp, dn) if kind == 'dice' else lp, adv)
                p = RL.maml_adapt_policy(l, p, PO.INNER_LR, False)
            n = int(inp['qry']['count'][t])
            lp = RL.policy_log_prob(p, inp['qry']['states'][t, :n], inp['qry']['actions'][t, :n], torch.tanh)
            adv, dn = inp['qry']['adv'][t, :n].reshape(-1, 1), inp['qry']['done'][t, :n].reshape(-1, 1)
            if kind == 'ppo':
                l = RL.ppo_policy_loss(lp, lp.detach(), adv, PO.CLIP)
            else:
                l = RL.a2c_policy_loss(RL.dice_log_probs(lp, dn) if kind == 'dice' else lp, adv)
            gsum += torch.cat([g.reshape(-1) for g in torch.autograd.grad(l, list(p0.values()))])
            assert abs(float(loss[t]) - float(l)) <= 1e-12 * max(1.0, abs(float(l)))
            assert _rel(th[t], torch.cat([x.detach().reshape(-1) for x in p.values()])) <= 1e-13
        assert _rel(grad, gsum) <= 1e-12
    # update with one epoch is adapt; with two, the second a2c epoch is adapt from the first one's result
    s0 = PO.sup_k(inp, 0)
    u1, l1 = o.update(inp['theta'], s0, epochs=1)
    a1, la = o.adapt(inp['theta'], s0)
    assert torch.equal(u1, a1) and torch.equal(l1[:, 0], la)
    u2, l2 = o.update(inp['theta'], s0, epochs=2)
    for t in range(inp['T']):
        one = {k: v[t:t + 1] for k, v in s0.items()}
        a2, lb = o.adapt(a1[t], one)
        assert _rel(u2[t], a2[0]) <= 1e-14 and abs(float(l2[t, 1]) - float(lb[0])) <= 1e-14 * max(1.0, abs(float(lb[0])))


@pytest.mark.parametrize('name', list(PO.CASES))
def test_case_inputs_seed_margin_and_nonzero_blocks(name):
    S, A, H1, H2, act, T, B, count, base = PO.CASES[name]
    seed, m = PO.find_seed(name)
    assert seed == PO.SEEDS[name], f'{name}: the search gives seed {seed} (margin {m}), the tests use {PO.SEEDS[name]}'
    inp, ref, margin = PO.reference(name)
    if act == 'relu':
        assert m >= PO.MARGIN and margin == m, (m, margin)          # the full walk meets the same points as the search
    else:
        assert margin == math.inf
    # counts as the issue states them
    for c in list(inp['sup']['count']) + [inp['qry']['count']]:
        c = c.tolist()
        assert c == list(count) if count is not None else (c[0] == B and all(B // 2 <= x < B for x in c[1:]))
    sl = PO.block_slices(S, A, H1, H2)
    th = inp['theta']

    def nonzero(vec, skip=()):
        for k, s in sl.items():
            if k not in skip:
                assert float(torch.as_tensor(vec)[..., s].norm()) > 0, (name, k)
    body = ('W1', 'b1', 'W2', 'b2')
    for ho in (False, True):
        for t in range(T):
            nonzero(ref['adapt', ho][0][t] - th, body if ho else ())
        assert not ho or all(torch.equal(ref['adapt', True][0][:, sl[k]], th[sl[k]].expand(T, -1)) for k in body)
    for K in (1, 2):
        f, g = ref['trpo', K, 'fisher'], ref['trpo', K, 'general']
        assert abs(float(f['kl'])) < 1e-12 and float(g['kl']) > 1e-6
        for r in (f, g):
            for vec in [r['grad']] + r['hv']:
                nonzero(vec)
        nonzero(g['kl_grad'])
    for key, val in ref.items():
        if key[0] == 'meta':
            nonzero(val[2])
            for t in range(T):
                nonzero(val[1][t] - th, body if key[2] else ())
        if key[0] == 'update':
            for t in range(T):
                nonzero(val[0][t] - th)
    assert all(bool(torch.isfinite(torch.as_tensor(x)).all()) for val in ref.values() if isinstance(val, tuple) for x in val)
