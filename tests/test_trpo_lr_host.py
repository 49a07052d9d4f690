"""The TRPO calls with per-parameter, fixed inner-loop step sizes, the parts that need no GPU:
(a) the recursions the kernels implement (tests/trpo_lr_oracle.py::closed_form) against fp64 autograd of the whole surrogate / KL:
    gradients to 1e-12 and curvature products to 1e-10 -- both sides are fp64 evaluations of the same expression, so a miss is a
    formula error, not noise;
(b) the Fisher form stays exact under vector steps (new == old);
(c) the discriminating condition of the GPU test's vector, from the oracle alone: the wrong-order adjoint lam - d (.) (H lam) and the
    scalar call at the mean step miss the GPU bars by a factor of 10 and more;
(d) the host logic: row mapping, refusal of a learnable wrapper under the function's name, acceptance of a fixed one (engine replaced by a
    test double, as in tests/test_rl_boundary.py), the drivers' flags;
(e) the argument checks of the new C entries, which run before any HIP call."""
import ctypes as C
from copy import deepcopy

import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as cf_rl
from oracle import rl_ref as RL
from test_rl_boundary import FakeEngine, ReplayRunner
import trpo_lr_oracle as O


def _both(name, wrong_order=False):
    c = O.make_case(name)
    ref = O.reference(name)
    args = (c['net'], c['theta'], c['replays'], c['olds'], c['lr_vec'], c['rows'], c['params'])
    return c, ref, O.closed_form(*args, vs=ref['vs'], wrong_order=wrong_order)


def _close(got, want, tol):
    scale = max(1.0, float(want.abs().max()))
    return float((got - want).abs().max()) <= tol * scale


# ------------------------------------------------------------------------------------------------------------- (a), (b)
@pytest.mark.parametrize('name', ['relu_k1', 'relu_k2', 'relu_k3', 'tanh_k1', 'anil_tanh_k1', 'anil_relu_k2', 'anil_tanh_k2_ragged', 'odd_t3'])
def test_closed_form_is_fp64_autograd(name):
    """ReLU and tanh, K = 1, 2, 3, a row per update, a frozen tensor (``mean.0.`` at 0 in every case), and ANIL's asymmetry (old policies
    adapted with d (.) head mask, the surrogate re-adapts with d)."""
    c, ref, got = _both(name)
    assert bool((c['lr_vec'][:, c['net'].mask(('mean.0.',))] == 0).all())
    assert len(set(c['rows'])) == len(c['rows'])                                    # K > 1: every update its own row
    assert _close(got['grad'], ref['grad'], 1e-12)
    assert _close(got['kl_grad'], ref['kl_grad'], 1e-12)
    if c['anil']:
        assert ref['kl'] > 1e-6 and float(ref['kl_grad'].norm()) > 0                # new != old
        for g, w in zip(got['general'], ref['hvp']):
            assert _close(g, w, 1e-10)
        assert not _close(got['fisher'][0], ref['hvp'][0], 1e-6)                    # ... where the Fisher form is not the Hessian
    else:
        # new == old: the exact KL Hessian product (double backward) IS J^T F J v, under a non-uniform vector with a frozen tensor too
        assert ref['kl'] < 1e-20 and float(ref['kl_grad'].abs().max()) < 1e-12
        for f, g, w in zip(got['fisher'], got['general'], ref['hvp']):
            assert _close(f, w, 1e-10) and _close(g, w, 1e-10)
    # frozen, not detached: theta_K keeps theta there, the gradient still reaches it (the cross-Hessian term)
    fm = c['net'].mask(('mean.0.',))
    assert all(torch.equal(t[fm], c['theta'][fm]) for t in got['theta_K'])
    assert float(ref['grad'][fm].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('name', ['relu_k1', 'relu_k2', 'tanh_k1', 'anil_tanh_k1', 'anil_relu_k1', 'anil_tanh_k2', 'anil_relu_k2'])
def test_gpu_vector_tells_the_wrong_adjoint_and_the_scalar_call_apart(name):
    """For the vector the GPU tests use (base * U(0.25, 4) per entry, ``mean.0.`` at 0, a second row at K = 2): D H on the adjoint side misses
    the oracle's gradient by >= 1e-3 and its product by >= 1e-2 -- 10x the GPU bars -- and the scalar call at the mean step misses both by
    >= 1e-2.  (With U(0.5, 1.5) the wrong product of relu_k1 is 4.6e-3 off: inside 10x the bar, hence the wider spread.)"""
    c, ref, wrong = _both(name, wrong_order=True)
    key = 'general' if c['anil'] else 'fisher'
    wg, wp = O.rel(wrong['grad'], ref['grad']), min(O.rel(x, y) for x, y in zip(wrong[key], ref['hvp']))
    mean = torch.full_like(c['lr_vec'], float(c['lr_vec'].mean()))
    sc = O.autograd_route(c['net'], c['theta'], c['replays'], c['olds'], mean, c['rows'], c['params'], ref['vs'])
    sg, sp = O.rel(sc['grad'], ref['grad']), min(O.rel(x, y) for x, y in zip(sc['hvp'], ref['hvp']))
    print(f'{name}: wrong-order grad {wg:.3e} product {wp:.3e}; mean-step scalar grad {sg:.3e} product {sp:.3e}')
    assert wg >= 1e-3 and wp >= 1e-2
    assert sg >= 1e-2 and sp >= 1e-2


def test_narrow_spread_would_not_discriminate():
    """Why the vector is not base * U(0.5, 1.5): there the wrong-order product of the fused case stays inside 10x the GPU bar."""
    c = O.make_case('relu_k1', spread=(0.5, 1.5))
    args = (c['net'], c['theta'], c['replays'], c['olds'], c['lr_vec'], c['rows'], c['params'])
    vs = O.directions(c['net'])
    ref = O.autograd_route(*args, vs)
    wrong = O.closed_form(*args, vs=vs, wrong_order=True)
    assert O.rel(wrong['fisher'][0], ref['hvp'][0]) < 1e-2


# ------------------------------------------------------------------------------------------------------------- (d)
class VectorEngine(FakeEngine):
    """tests/test_rl_boundary.py's double, taking a [P] row in ``adapt`` and a [rows, P] table with ``step_lr_row`` in the TRPO calls."""

    def __init__(self, activation):
        super().__init__(activation)
        self.calls = []

    def adapt(self, theta, states, actions, adv, count, lr, head_only=False):
        self.calls.append(('adapt', lr))
        return super().adapt(theta, states, actions, adv, count, lr.double() if torch.is_tensor(lr) else lr, head_only)

    def _surr(self, th, sup, qry, old_loc, old_scale, lr):
        if not torch.is_tensor(lr):
            return super()._surr(th, sup, qry, old_loc, old_scale, lr)
        T = qry['states'].shape[0]
        loss, kl = 0.0, 0.0
        for t in range(T):
            new = th
            for k in range(sup['states'].shape[0]):
                new, _ = self._inner(new, sup['states'][k, t], sup['actions'][k, t], sup['adv'][k, t], int(sup['count'][k, t]),
                                     lr[self._rows[k]].double(), False, True)
            n = int(qry['count'][t])
            loc, scale = RL.policy_loc_scale(self._p(new), qry['states'][t, :n].double(), self.act)
            ol, os_ = old_loc[t, :n].double(), old_scale[t].double()
            kl = kl + RL.normal_kl(loc, scale, ol, os_).mean()
            old_lp = RL.normal_log_prob(ol, os_, qry['actions'][t, :n].double()).mean(dim=1, keepdim=True)
            new_lp = RL.normal_log_prob(loc, scale, qry['actions'][t, :n].double()).mean(dim=1, keepdim=True)
            loss = loss + RL.trpo_policy_loss(new_lp, old_lp, qry['adv'][t, :n].double().reshape(-1, 1))
        return loss / T, kl / T

    def surrogate(self, theta, sup, qry, old_loc, old_scale, inner_lr, want_grad, step_lr_row=None):
        self.calls.append(('surrogate', inner_lr, step_lr_row))
        self._rows = [0] * sup['states'].shape[0] if step_lr_row is None else list(step_lr_row)
        return super().surrogate(theta, sup, qry, old_loc, old_scale, inner_lr, want_grad)

    def fvp(self, sup, qry, inner_lr, damping, v, step_lr_row=None):
        self.calls.append(('fvp', inner_lr, step_lr_row))
        return super().fvp(sup, qry, inner_lr, damping, v)


@pytest.fixture
def vector_engine(monkeypatch):
    engines = {}
    monkeypatch.setattr(cf.DiagNormalPolicy, 'engine', lambda self: engines.setdefault(self.activation, VectorEngine(self.activation)))
    return engines


def _cpu_policy(net, flat):
    pol = cf.DiagNormalPolicy(net.S, net.A, list(net.H), activation=net.act_name)
    pol.load_flat(flat.float())
    return pol


def _fixed(pol, table):
    t = table.float()
    return cf.MAML(pol, lr=cf.InnerLR(pol, t, per='parameter', steps=t.shape[0], learnable=False))


def test_rows_and_refusal():
    """Adapt step k reads row k of a table with a row per step, row 0 of a one-row table; anything else is refused; a wrapper whose steps
    require grad is refused under the calling function's name, and the text says what is accepted."""
    assert cf_rl._lr_step_rows(1, 3) == [0, 0, 0] and cf_rl._lr_step_rows(3, 3) == [0, 1, 2]
    with pytest.raises(ValueError, match='adapt_steps'):
        cf_rl._lr_step_rows(2, 3)
    pol = cf.DiagNormalPolicy(2, 2)
    assert cf_rl._trpo_lr_table(pol, 'x') is None and cf_rl._trpo_lr_table(cf.MAML(pol, lr=0.1), 'x') is None
    fixed = cf.MAML(pol, lr=cf.InnerLR(pol, 0.1, per='tensor', steps=2, frozen=('mean.0.',)))
    table = cf_rl._trpo_lr_table(fixed, 'x')
    assert tuple(table.shape) == (2, 10604) and not table.requires_grad and table.dtype == torch.float32
    assert bool((table[:, 2:302] == 0).all()) and bool((table[:, :2] == 0.1).all()) and bool((table[:, 402:] == 0.1).all())
    for kw in (dict(learnable=True), dict(learnable=True, frozen=('mean.0.',))):
        learn = cf.MAML(pol, lr=cf.InnerLR(pol, 0.1, per='tensor', **kw))
        for name in ('fast_adapt_trpo', 'fast_adapt_trpo_tasks', 'trpo_update', 'meta_optimize_trpo', 'meta_surrogate_loss', 'evaluate_trpo'):
            with pytest.raises(ValueError, match=name) as e:
                cf_rl._trpo_lr_table(learn, name)
            assert "params['inner_lr']" in str(e.value) and 'fixed' in str(e.value).lower()
    with pytest.raises(ValueError, match='meta_optimize_trpo'):
        cf.meta_optimize_trpo(dict(O.PARAMS), learn, cf.LinearValue(2, 2), [], [])
    with pytest.raises(ValueError, match='fast_adapt_trpo'):
        cf.fast_adapt_trpo(None, learn, cf.LinearValue(2, 2), dict(O.PARAMS))
    # a number with allow_nograd around a policy with a frozen parameter is a fixed table as well
    frozen = cf.DiagNormalPolicy(2, 2)
    frozen.mean[0].weight.requires_grad_(False)
    t = cf_rl._trpo_lr_table(cf.MAML(frozen, lr=0.1, allow_nograd=True), 'x')
    assert tuple(t.shape) == (1, 10604) and bool((t[0, 2:202] == 0).all()) and bool((t[0, 202:] == 0.1).all())


@pytest.mark.parametrize('name', ['relu_k2', 'anil_tanh_k2'])
def test_fixed_wrapper_is_accepted_and_reads_its_rows(name, vector_engine):
    """fast_adapt_trpo, trpo_update and meta_surrogate_loss / meta_optimize_trpo's context with ``MAML(policy, lr=InnerLR(fixed))`` on the
    engine double: adapt step k is handed row k of the table (the ANIL walk with head_only), the surrogate the whole table with the rows,
    and the results are the oracle's."""
    c = O.make_case(name)
    net, K = c['net'], len(c['rows'])
    pol = _cpu_policy(net, c['theta'])
    if c['anil']:
        pol.features_no_grad = True                                   # what DiagNormalPolicyANIL.turn_off_body_grads() sets
    maml = _fixed(pol, c['lr_vec'])
    eng = pol.engine()
    learner, _, replays, _, _ = cf.fast_adapt_trpo(ReplayRunner(c['replays'][0]), deepcopy(maml), cf.LinearValue(2, 2), c['params'])
    adapts = [x for x in eng.calls if x[0] == 'adapt']
    assert len(adapts) == K and all(torch.equal(a[1], c['lr_vec'][k].float()) for k, a in enumerate(adapts))
    assert O.rel(cf_rl._unwrap(learner).flat().double(), c['olds'][0]) < 1e-5
    # trpo_update walks the rows like the step-wise learner's adapt
    del eng.calls[:]
    one = cf_rl.trpo_update(c['replays'][0][0], deepcopy(maml), cf.LinearValue(2, 2), 123.0, 0.99, 1.0)
    two = cf_rl.trpo_update(c['replays'][0][1], one, cf.LinearValue(2, 2), 123.0, 0.99, 1.0)
    assert [torch.equal(a[1], c['lr_vec'][k].float()) for k, a in enumerate(eng.calls)] == [True, True]
    assert O.rel(cf_rl._unwrap(two).flat().double(), c['olds'][0]) < 1e-5
    with pytest.raises(ValueError, match='trpo_update'):
        cf_rl.trpo_update(c['replays'][0][1], two, cf.LinearValue(2, 2), 123.0, 0.99, 1.0)
    # the surrogate: the table as it is (no head mask), with the rows
    pol.features_no_grad = False
    del eng.calls[:]
    olds = [_cpu_policy(net, o) for o in c['olds']]
    loss, kl = cf.meta_surrogate_loss(c['replays'], olds, maml, cf.LinearValue(2, 2), c['params'])
    (call,) = eng.calls
    assert call[0] == 'surrogate' and torch.equal(call[1], c['lr_vec'].float()) and list(call[2]) == c['rows']
    ref = O.reference(name)
    assert abs(float(loss) - ref['loss']) < 1e-5 and abs(float(kl) - ref['kl']) < 1e-5 * max(ref['kl'], 1e-3)
    with pytest.raises(ValueError, match='adapt_steps'):                  # a 2-row table under 3 adapt steps
        cf.fast_adapt_trpo(ReplayRunner(c['replays'][0] * 2), deepcopy(maml), cf.LinearValue(2, 2), dict(c['params'], adapt_steps=3))


def test_driver_flags_build_the_wrapper():
    from exploring_meta_amd.rl import maml_trpo
    pol = cf.DiagNormalPolicy(2, 2)
    p = dict(maml_trpo.params)
    assert maml_trpo.wrap_policy(pol, p) is pol                            # the defaults build what they built before
    w = maml_trpo.wrap_policy(pol, dict(p, adapt_steps=2, inner_lr_per='tensor', per_step_lr=True, freeze=['mean.0.']))
    assert isinstance(w, cf.MAML) and w.module is pol
    lr = w.lr
    assert isinstance(lr, cf.InnerLR) and not lr.learnable and lr.steps == 2 and lr.per == 'tensor' and lr.frozen == ('mean.0.',)
    assert not any(q is lr.values for q in w.parameters())                 # fixed: nothing for an optimiser, nothing that requires grad
    assert cf_rl._trpo_lr_table(w, 'x').shape[0] == 2
    assert isinstance(maml_trpo.wrap_policy(pol, dict(p, freeze=['mean.0.'])).lr, cf.InnerLR)
    anil = cf.DiagNormalPolicyANIL(2, 2, 100)
    t = cf_rl._trpo_lr_table(maml_trpo.wrap_policy(anil, dict(p, inner_lr_per='tensor', freeze=['body.0.'])), 'x')
    assert bool((t[0, :2] == p['inner_lr']).all()) and bool((t[0, 2:302] == 0).all())         # the engine's order: sigma first
    import argparse
    parser = argparse.ArgumentParser()
    maml_trpo.add_lr_flags(parser)
    args = parser.parse_args(['--inner_lr_per', 'parameter', '--per_step_lr', '--freeze', 'mean.0.', 'sigma'])
    assert (args.inner_lr_per, args.per_step_lr, args.freeze) == ('parameter', True, ['mean.0.', 'sigma'])
    assert not any(a.dest == 'learn_inner_lr' for a in parser._actions)


# ------------------------------------------------------------------------------------------------------------- (e)
def test_argument_errors_come_before_any_hip_call():
    """MI_ERR_ARG with a text naming the entry and the value; no device is touched (this runs without one: the pointers are host
    addresses the library must not follow)."""
    lib = _lib.load()
    desc = _lib.MiPolicyDesc(2, 2, 100, 100, 0)
    h = C.c_void_p()
    assert lib.mi_policy_create(C.byref(desc), 0, C.byref(h)) == 0
    ptr = C.c_void_p(64)
    bad_hi, bad_lo = (C.c_int32 * 2)(0, 2), (C.c_int32 * 2)(-1, 0)
    big = 1 << 40

    def surrogate(vec=ptr, rows=2, sr=None, steps=2, tasks=3, batch=4):
        return lib.mi_trpo_surrogate_steps_lr(h, None, ptr, steps, ptr, ptr, ptr, None, ptr, ptr, ptr, None, ptr, ptr, tasks, batch, vec, rows, sr,
                                              ptr, ptr, ptr, ptr, big)

    def fvp(vec=ptr, rows=2, sr=None, steps=2, tasks=3, batch=4):
        return lib.mi_trpo_fvp_steps_lr(h, None, steps, ptr, ptr, None, ptr, None, tasks, batch, vec, rows, sr, 1e-5, ptr, ptr, ptr, big)

    def prepare(vec=ptr, rows=2, sr=None, steps=2, tasks=3, batch=4):
        return lib.mi_trpo_kl_prepare_steps_lr(h, None, steps, ptr, ptr, None, ptr, None, ptr, ptr, tasks, batch, vec, rows, sr, ptr, ptr, big)

    def general(vec=ptr, rows=2, sr=None, steps=2, tasks=3, batch=4):
        return lib.mi_trpo_fvp_general_steps_lr(h, None, steps, ptr, ptr, None, ptr, None, ptr, tasks, batch, vec, rows, sr, 1e-5, ptr, ptr, ptr, big)
    for name, call in (('mi_trpo_surrogate_steps_lr', surrogate), ('mi_trpo_fvp_steps_lr', fvp), ('mi_trpo_kl_prepare_steps_lr', prepare),
                       ('mi_trpo_fvp_general_steps_lr', general)):
        for kw, text in ((dict(vec=None), 'lr_vec'), (dict(rows=0), 'lr_rows 0'), (dict(rows=-3), 'lr_rows -3'),
                         (dict(sr=bad_hi), 'step_lr_row[1] 2'), (dict(sr=bad_lo), 'step_lr_row[0] -1'), (dict(steps=0), 'steps 0'),
                         (dict(tasks=0), 'tasks 0'), (dict(batch=0), 'batch 0')):
            assert call(**kw) == -1, (name, kw)
            msg = lib.mi_policy_last_error(h).decode()
            assert name in msg and text in msg, msg
    rc = lib.mi_policy_adapt_lr(h, None, ptr, 0, ptr, ptr, ptr, None, 3, 4, None, 0, ptr, None, ptr, big)
    assert rc == -1 and 'mi_policy_adapt_lr' in lib.mi_policy_last_error(h).decode() and 'lr_vec' in lib.mi_policy_last_error(h).decode()
    rc = lib.mi_policy_adapt_lr(h, None, ptr, 0, ptr, ptr, ptr, None, 0, 4, ptr, 0, ptr, None, ptr, big)
    assert rc == -1 and 'mi_policy_adapt_lr: tasks 0' in lib.mi_policy_last_error(h).decode()
    # the scalar entries' own checks still come first in the vector entries, under the entry's name
    rc = lib.mi_trpo_surrogate_steps_lr(h, None, None, 2, ptr, ptr, ptr, None, ptr, ptr, ptr, None, ptr, ptr, 3, 4, ptr, 2, None, ptr, ptr, ptr, ptr, big)
    assert rc == -1 and 'mi_trpo_surrogate_steps_lr: null argument' in lib.mi_policy_last_error(h).decode()
    # workspaces: the MAML-TRPO plan does not grow; the general plan grows by [steps][tasks][P] floats behind the scalar plan
    n, m = C.c_size_t(5), C.c_size_t()
    assert lib.mi_trpo_steps_lr_workspace_bytes(h, 3, 40, 2, 0, C.byref(n)) == -1 and n.value == 5
    assert lib.mi_trpo_general_steps_lr_workspace_bytes(h, 3, 40, 2, 0, C.byref(n)) == -1 and n.value == 5
    assert lib.mi_trpo_steps_lr_workspace_bytes(h, 3, 40, 2, 2, C.byref(n)) == 0 and lib.mi_trpo_steps_workspace_bytes(h, 3, 40, 2, C.byref(m)) == 0
    assert n.value == m.value
    assert lib.mi_trpo_general_steps_lr_workspace_bytes(h, 3, 40, 2, 2, C.byref(n)) == 0
    assert lib.mi_trpo_general_steps_workspace_bytes(h, 3, 40, 2, C.byref(m)) == 0
    assert 0 <= n.value - m.value - 4 * 2 * 3 * 10604 < 256
    lib.mi_policy_destroy(h)
