"""CPU side of the step-wise policy learner: the inputs of tests/test_gpu_policy_learner.py (seeds, ReLU margins), the autograd wiring of
``DiagNormalPolicy.density(theta=)`` / ``MAML(policy)`` against plain autograd with the engine replaced by an fp64 autograd test double
(tests/policy_learner_cases.AutogradEngine: forward / vjp / hvp), and calc_cl_metrics against values worked out by hand."""
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

import policy_learner_cases as LC
import policy_shapes_oracle as PO
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as PR
from oracle import rl_ref as RL


# --------------------------------------------------------------------------------------------------- cases
@pytest.mark.parametrize('name', list(LC.EXTRA))
def test_seed_search_gives_the_pinned_seed(name):
    seed, margin = LC.find_seed(name)
    assert seed == LC.SEEDS[name], (seed, margin)
    assert margin >= PO.MARGIN


@pytest.mark.parametrize('name', LC.NAMES)
def test_relu_margins_and_reference_blocks(name):
    """Every ReLU pre-activation met at theta and at the adapted parameters stays MARGIN away from the kink; the structural zeros of the
    references are exact (sigma everywhere, b3 of the Hessian product, the body and the whole Hessian product in head_only mode), and
    every block the GPU tests divide by is either nonzero or exactly zero (dead ReLU units at the 1-wide layers)."""
    inp, ref, margin = LC.reference(name)
    if inp['activation'] == 'relu':
        assert margin >= PO.MARGIN, margin
    sl = PO.block_slices(inp['S'], inp['A'], *inp['H'])
    for per_task in (False, True):
        for head_only in (False, True):
            g, h, ld = ref[per_task, head_only]
            assert bool(torch.isfinite(g).all() and torch.isfinite(h).all() and torch.isfinite(ld).all())
            assert float(g[:, sl['sigma']].abs().max()) == 0.0 and float(h[:, sl['sigma']].abs().max()) == 0.0
            assert float(h[:, sl['b3']].abs().max()) == 0.0
            assert float(g[:, sl['W3']].norm()) > 0.0 and float(g[:, sl['b3']].norm()) > 0.0 and float(ld.norm()) > 0.0
            if head_only:
                assert float(h.abs().max()) == 0.0
                assert all(float(g[:, sl[k]].abs().max()) == 0.0 for k in ('W1', 'b1', 'W2', 'b2'))
            for t in range(inp['T']):
                assert float(ld[t, int(inp['batch']['count'][t]):].abs().max() if int(inp['batch']['count'][t]) < inp['B'] else 0.0) == 0.0
    if name not in ('min_1x1',):                              # (its single hidden units are dead on some tasks: exact zeros there)
        g, h, _ = ref[False, False]
        assert all(float(g[t, sl[k]].norm()) > 0.0 for t in range(inp['T']) for k in ('W1', 'b1', 'W2', 'b2'))
        assert all(float(h[t, sl[k]].norm()) > 0.0 for t in range(inp['T']) for k in ('W1', 'b1', 'W2', 'b2', 'W3'))


def test_cases_cover_the_fused_range_and_its_outside():
    shapes = {n: LC.shape(n) for n in LC.NAMES}
    fused = lambda s: s[2] <= 128 and s[3] <= 128 and s[0] <= 16 and s[1] <= 6
    assert not fused(shapes['wide_160x132']) and all(fused(s) for n, s in shapes.items() if n != 'wide_160x132')
    assert shapes['limits_128'][:4] == (16, 6, 128, 128) and shapes['h2_65'][3] == 65
    for n in ('default_relu', 'default_tanh', 'metaworld_relu'):
        assert shapes[n][5:] == (2, 2 * 16 + 1)


# --------------------------------------------------------------------------------------------------- autograd wiring on a test double
@pytest.fixture
def double_engine(monkeypatch):
    engines = {}

    def engine(self):
        key = (self.input_size, self.output_size, self.hiddens, self.activation)
        if key not in engines:
            engines[key] = LC.AutogradEngine(self.input_size, self.output_size, self.hiddens, self.activation)
        return engines[key]
    monkeypatch.setattr(cf.DiagNormalPolicy, 'engine', engine)
    return engines


def _policy(inp, anil=False):
    S, A, H = inp['S'], inp['A'], inp['H']
    pol = cf.DiagNormalPolicyANIL(S, A, H[1], list(H)) if anil else cf.DiagNormalPolicy(S, A, list(H), activation=inp['activation'])
    pol = pol.double()
    off = 0
    with torch.no_grad():
        for p in pol._engine_params():
            p.copy_(inp['theta'][off:off + p.numel()].view_as(p))
            off += p.numel()
    return pol


_rows = LC.rows


@pytest.mark.parametrize('first_order', [False, True])
@pytest.mark.parametrize('name,anil', [('k8_12x50', False), ('odd_5x3', False), ('odd_5x3', True)])
def test_stepwise_chain_equals_plain_autograd(double_engine, name, anil, first_order):
    """``learner = MAML(policy, lr).clone()``; two ``learner.adapt(loss)``; ``query_loss.backward()``: fast weights, loss and the gradient
    in the policy's parameters equal plain autograd (1e-10: fp64 on both sides).  Second order runs one hvp per adapt step (and one more
    vjp each: the cotangent of that step's loc through its loss), first order none.  anil: DiagNormalPolicyANIL with turn_off_body_grads() during the adaptation (head_only), back on for the query."""
    inp = PO.make_inputs(name)
    pol = _policy(inp, anil)
    sups, qry, t, lr = [PO.sup_k(inp, 0), PO.sup_k(inp, 1)], inp['qry'], 1, PO.INNER_LR
    learner = cf.MAML(pol, lr=lr, first_order=first_order).clone()
    assert learner.__dict__['_fast'] is None
    if anil:
        pol.turn_off_body_grads()
    for sup in sups:
        s, a, adv = _rows(sup, t)
        learner.adapt(-(learner.log_prob(s, a) * adv).mean(), allow_unused=anil)
    if anil:
        pol.turn_on_body_grads()
    s, a, adv = _rows(qry, t)
    loss = -(learner.log_prob(s, a) * adv).mean()
    loss.backward()
    th_ref, loss_ref, grad_ref = LC.plain_chain(inp, sups, qry, t, lr, first_order, anil)
    got = torch.cat([p.grad.reshape(-1) for p in pol._engine_params()])
    rel = lambda x, y: float((x - y).norm() / y.norm())
    assert rel(learner.fast_weights().detach(), th_ref) < 1e-10
    assert abs(float(loss.detach()) - float(loss_ref)) < 1e-10 * max(1.0, abs(float(loss_ref)))
    assert rel(got, grad_ref) < 1e-10
    calls = next(iter(double_engine.values())).calls
    assert calls.count('hvp') == (0 if first_order else 2) and calls.count('vjp') == (3 if first_order else 5)


def test_kl_hessian_vector_product_and_third_order(double_engine):
    """g = grad(mean KL, theta, create_graph=True); grad(g . v, theta) equals plain autograd; one more derivative raises."""
    inp = PO.make_inputs('odd_5x3')
    pol = _policy(inp)
    s, _, _ = _rows(inp['qry'], 0)
    theta = pol.flat_parameters()
    old = torch.distributions.Normal(pol.density(s).loc + 0.1, torch.full((inp['A'],), 0.7, dtype=torch.float64))
    v = PO._f32(torch.randn(theta.numel(), generator=torch.Generator().manual_seed(3), dtype=torch.float64))

    def hvp(density):
        kl = torch.distributions.kl_divergence(density, old).mean()
        (g,) = torch.autograd.grad(kl, theta, create_graph=True)
        return g, torch.autograd.grad((g * v).sum(), theta, create_graph=True)[0]
    g, hv = hvp(pol.density(s, theta=theta))
    eng = next(iter(double_engine.values()))
    loc = eng._loc(theta, s)
    g_ref, hv_ref = hvp(torch.distributions.Normal(loc, torch.exp(torch.clamp(theta[:inp['A']], min=math.log(1e-6)))))
    assert float((g - g_ref).norm() / g_ref.norm()) < 1e-10 and float((hv - hv_ref).norm() / hv_ref.norm()) < 1e-10
    with pytest.raises(RuntimeError, match='third derivative'):
        torch.autograd.grad(hv.sum(), theta)


def test_bare_policy_and_unadapted_learner_stay_detached(double_engine):
    """policy.density / log_prob / policy(state) carry no graph; a MAML wrapper that was never adapted samples through the bare policy
    and holds no state; its log_prob has the bare policy's value and a graph only while grad mode is on."""
    inp = PO.make_inputs('odd_5x3')
    pol = _policy(inp)
    s, a, _ = _rows(inp['qry'], 0)
    lp = pol.log_prob(s, a)
    assert not lp.requires_grad and not pol.density(s).loc.requires_grad and not pol(s).requires_grad
    learner = cf.MAML(pol, lr=0.1)
    lp2 = learner.log_prob(s, a)
    assert lp2.requires_grad and learner.__dict__['_fast'] is None
    assert torch.allclose(lp2.detach(), lp, rtol=0, atol=1e-6)      # (the bare path runs in fp32; equal bits: the GPU test)
    with torch.no_grad():
        assert not learner.log_prob(s, a).requires_grad
    torch.manual_seed(0)
    x = learner(s)
    torch.manual_seed(0)
    assert torch.equal(x, pol(s)) and not x.requires_grad
    learner.adapt(-lp2.mean())
    assert not learner(s).requires_grad and learner.log_prob(s, a).requires_grad
    import copy
    twin = copy.deepcopy(learner)                              # adapted fast weights copy as values
    assert torch.equal(twin.fast_weights(), learner.fast_weights().detach()) and twin.module is not pol
    assert torch.equal(learner.adapted_policy().flat().double(), learner.fast_weights().detach().float().double())


def test_vpg_a2c_loss_is_differentiable_on_a_wrapper(double_engine, monkeypatch):
    """reference cl_rl.py:71-75: learner.adapt(vpg_a2c_loss(episodes, learner, ...)).  Value: the bare policy's; dice stays value only."""
    monkeypatch.setattr(PR, 'device', torch.device('cpu'))
    inp = PO.make_inputs('min_1x1')
    pol = _policy(inp)
    s, a, adv = _rows(PO.sup_k(inp, 0), 0)
    monkeypatch.setattr(PR, 'compute_advantages', lambda *args: adv.numpy())
    n = s.shape[0]
    ep = dict(states=s, actions=a, rewards=torch.zeros(n, 1), dones=torch.zeros(n, 1), next_states=s)
    learner = cf.MAML(pol, lr=PO.INNER_LR)
    bare = PR.vpg_a2c_loss(ep, pol, None, 0.99, 1.0)
    loss = PR.vpg_a2c_loss(ep, learner, None, 0.99, 1.0)
    assert not bare.requires_grad and loss.requires_grad and float(bare) == pytest.approx(float(loss), rel=1e-6)
    assert not PR.vpg_a2c_loss(ep, learner, None, 0.99, 1.0, dice=True).requires_grad
    learner.adapt(loss)
    o = PO.Oracle(inp['S'], inp['A'], inp['H'], inp['activation'])
    th_ref, _ = o.adapt(inp['theta'], PO.sup_k(inp, 0), lr=PO.INNER_LR)
    assert float((learner.fast_weights().detach() - th_ref[0]).abs().max()) < 1e-6      # (adv passes through fp32 in vpg_a2c_loss)


# --------------------------------------------------------------------------------------------------- continual-learning metrics
def test_calc_cl_metrics_by_hand():
    """3 x 3, rows = adapted on, columns = evaluated on.
    av_acc: (0.9 + 0.6 + 0.8 + 0.5 + 0.7 + 1.0) / 6 = 0.75;  fwt: (0.2 + 0.1 + 0.3) / 3 = 0.2;
    bwt: rows 1, 2 x columns 0, 1 against the diagonal: (0.6 - 0.9) + (0.8 - 0.8) + (0.5 - 0.9) + (0.7 - 0.8) = -0.8, / 3 = -0.2667:
    rem = 1 - 0.2667, bwt_plus = 0.  Second matrix: bwt = ((0.7 - 0.5) + 0 + (0.9 - 0.5) + (0.8 - 0.6)) / 3 = 0.2667: rem = 1."""
    from exploring_meta_amd.utils.cl_metrics import calc_cl_metrics
    m = calc_cl_metrics(np.array([[0.9, 0.2, 0.1], [0.6, 0.8, 0.3], [0.5, 0.7, 1.0]]))
    assert m['av_acc'] == pytest.approx(0.75) and m['fwt'] == pytest.approx(0.2)
    assert m['rem'] == pytest.approx(1 - 0.8 / 3) and m['bwt_plus'] == 0.0
    m = calc_cl_metrics([[0.5, 0.0, 0.3], [0.7, 0.6, 0.0], [0.9, 0.8, 0.4]])
    assert m['av_acc'] == pytest.approx(3.9 / 6) and m['fwt'] == pytest.approx(0.1)
    assert m['rem'] == 1.0 and m['bwt_plus'] == pytest.approx(0.8 / 3)
    with pytest.raises(ValueError):
        calc_cl_metrics(np.zeros((2, 3)))
