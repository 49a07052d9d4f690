"""Per-parameter, learnable inner-loop step sizes in the policy's fused calls (mi_policy_meta_batch_lr / mi_policy_update_lr,
include/mi_maml.h) on the GPU: against the scalar calls (uniform vectors), the fp64 oracle with the update
p - lr[k] * g (tests/policy_lr_oracle.py), at an odd parameter count, the calls' invariants, argument errors, and the Python surface
(InnerLR around a policy, fast_adapt_*_tasks, the step-wise learner, the maml_ppo driver, TRPO's refusal).
Shapes: the replays of tests/test_gpu_rl.py::test_policy_meta_batch_vpg_ppo (2-100-100-2, T = 3, 2 adapt steps, 5 episodes of 12-15 steps)
and one odd policy, 3-19-33-1 (P = 771)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.engine import PolicyEngine, _ptr, _stream
from gpu_utils import rel_err, report
import adapt_tasks_cases as AC
import policy_lr_oracle as O

pytestmark = pytest.mark.gpu

KIND = {'a2c': 0, 'ppo': 1, 'dice': 2}


def _f(x):
    return x.float().cuda().contiguous()


def _batch(b):
    return dict(states=_f(b['states']), actions=_f(b['actions']), adv=_f(b['adv']), done=_f(b['done']),
                count=b['count'].to(torch.int32).cuda().contiguous())


@functools.lru_cache(maxsize=None)
def _setup(act, algo):
    """(inputs, engine, theta, sup, qry on the device) for the Particles2D replays; shared, read-only."""
    inp = O.particle_replays(act, algo)
    eng = PolicyEngine(inp['S'], inp['A'], inp['H'], activation=act)
    assert eng.param_count == inp['theta'].numel()
    return inp, eng, _f(inp['theta']), _batch(inp['sup']), _batch(inp['qry'])


def _steps(kind, epochs=3, adapt_steps=2, per_step=True):
    e = epochs if kind == 'ppo' else 1
    step_batch = [b for b in range(adapt_steps) for _ in range(e)]
    return step_batch, ([b for b in step_batch] if per_step else None)


def _algo(kind):
    return 'ppo' if kind == 'ppo' else 'vpg'


def _bits(a, b):
    return a is not None and b is not None and a.shape == b.shape and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('kind,act,head_only,fo,lr', [('a2c', 'relu', False, True, 0.05), ('a2c', 'relu', False, False, 0.5),
                                                      ('dice', 'relu', False, False, 0.5), ('ppo', 'tanh', False, False, 0.0625),
                                                      ('a2c', 'tanh', True, False, 0.0625)])
@pytest.mark.parametrize('per_step', [False, True])
def test_uniform_vector_is_the_scalar_call_bit_for_bit(kind, act, head_only, fo, lr, per_step):
    """loss_out and theta_out equal the scalar call's bits at any step (0.05 here: the same multiply and subtract per element), and so does
    the first-order grad_out.  The second-order recursion drives the tangent pass with d lam where the scalar call scales H lam afterwards:
    the same bits when the step is a power of two, which is why those cases run at 0.5 / 0.0625."""
    inp, eng, theta, sup, qry = _setup(act, _algo(kind))
    step_batch, rows = _steps(kind, per_step=per_step)
    n_rows = 2 if per_step else 1
    P = eng.param_count
    for step, with_grad in ((0.05, False), (lr, True)):
        vec = torch.full((n_rows, P), step, device='cuda')
        want = eng.meta_batch(theta, sup, qry, step_batch, step, loss=kind, clip=0.1, head_only=head_only, first_order=fo, with_grad=with_grad)
        got = eng.meta_batch_lr(theta, sup, qry, step_batch, vec, rows, loss=kind, clip=0.1, head_only=head_only, first_order=fo,
                                with_grad=with_grad)
        torch.cuda.synchronize()
        assert _bits(got[0], want[0]) and _bits(got[1], want[1]), (kind, step)
        assert not torch.equal(got[1], theta.expand_as(got[1]))
        if with_grad:
            assert _bits(got[2], want[2]), (kind, step, rel_err(got[2].cpu().numpy(), want[2].cpu().numpy()))
            assert tuple(got[3].shape) == (n_rows, P) and bool(torch.isfinite(got[3]).all()) and float(got[3].abs().max()) > 0
        else:
            assert got[2] is None and got[3] is None


# ---------------------------------------------------------------------------------------------------------------- 2
ORACLE_CASES = {
    # name: (kind, act, head_only, first_order, base step, clip, per-step rows)
    'a2c-relu': ('a2c', 'relu', False, False, 0.05, 0.1, True),
    'a2c-relu-fo': ('a2c', 'relu', False, True, 0.05, 0.1, False),
    'a2c-tanh-head': ('a2c', 'tanh', True, False, 0.05, 0.1, True),
    'ppo-tanh-rows': ('ppo', 'tanh', False, False, 0.05, 0.1, True),
    'ppo-relu-clip': ('ppo', 'relu', False, False, 2.0, 0.02, False),
    'dice-relu': ('dice', 'relu', False, False, 0.05, 0.1, True),
}


@functools.lru_cache(maxsize=None)
def _oracle(name, fp64):
    """One oracle run per case and precision (never modified)."""
    kind, act, head_only, fo, base, clip, per_step = ORACLE_CASES[name]
    inp = O.particle_replays(act, _algo(kind))
    o = O.Oracle(inp['S'], inp['A'], inp['H'], act, torch.float64 if fp64 else torch.float32)
    step_batch, rows = _steps(kind, per_step=per_step)
    lr = O.lr_vector(o, base, 2 if per_step else 1, 5)
    return o.meta_lr(inp['theta'], inp['sup'], inp['qry'], step_batch, lr, rows, kind=kind, clip=clip, head_only=head_only, first_order=fo), lr


def _check_against(name, got, theta0, ref64, ref32, T):
    """The bars of test_policy_meta_batch_vpg_ppo for loss / parameter step / gradient; lr_grad by the project's rule."""
    loss, th, grad, lr_grad = (x.detach().cpu().double().numpy() for x in got)
    l64, th64, g64, lg64 = (x.numpy() for x in ref64)
    t0 = theta0.double().numpy()
    e_l = float(np.max(np.abs(loss - l64)))
    e_th = max(rel_err(th[t] - t0, th64[t] - t0) for t in range(T))
    e_g, e_lg = rel_err(grad, g64), rel_err(lr_grad, lg64)
    own = rel_err(ref32[3].double().numpy(), lg64)
    report(f'policy_lr[{name}]', loss_abs=e_l, theta_step_rel=e_th, grad_rel=e_g, lr_grad_rel=e_lg, lr_grad_oracle_fp32_rel=own)
    assert e_l < 2e-6 * max(1.0, float(np.max(np.abs(l64))))
    assert e_th < 1e-4 and e_g < 2e-4
    assert e_lg <= max(2e-4, 2 * own), (e_lg, own)


@pytest.mark.parametrize('name', list(ORACLE_CASES))
def test_non_uniform_steps_match_the_fp64_oracle(name):
    """base * U(0.5, 1.5) per entry with mean.0. at exactly 0 (seeded): loss, parameter step and meta-gradient at the bars of the scalar
    call's test; lr_grad within max(2e-4, 2 x the fp32 oracle's own error against fp64 on the same replays)."""
    kind, act, head_only, fo, base, clip, per_step = ORACLE_CASES[name]
    inp, eng, theta, sup, qry = _setup(act, _algo(kind))
    ref64, lr = _oracle(name, True)
    ref32, _ = _oracle(name, False)
    step_batch, rows = _steps(kind, per_step=per_step)
    got = eng.meta_batch_lr(theta, sup, qry, step_batch, _f(lr), rows, loss=kind, clip=clip, head_only=head_only, first_order=fo)
    torch.cuda.synchronize()
    _check_against(name, got, inp['theta'], ref64, ref32, inp['T'])
    o = O.Oracle(inp['S'], inp['A'], inp['H'], act)
    frozen = O.frozen_mask(o).cuda()
    assert torch.equal(got[1][:, frozen], theta[frozen].expand(inp['T'], -1))          # step exactly 0: bitwise unchanged
    if head_only:
        body = (o.head_mask() == 0).cuda()
        assert torch.equal(got[3][:, body], torch.zeros_like(got[3][:, body]))
        assert torch.equal(got[1][:, body], theta[body].expand(inp['T'], -1))
    else:
        assert float(got[3][:, frozen].abs().max()) > 0                                  # frozen is not detached


# ---------------------------------------------------------------------------------------------------------------- 3
ODD = dict(S=3, A=1, H=(19, 33), B=40, counts=[(37, 20, 1), (25, 33, 39), (31, 1, 38)])


@functools.lru_cache(maxsize=None)
def _odd(T, fp64):
    inp = O.random_inputs(ODD['S'], ODD['A'], ODD['H'], 3, ODD['B'], ODD['counts'], seed=23)
    if T == 1:
        inp = O.task_slice(inp, [1])                              # counts 20, 33, 1: every replay short of the batch, one with a single row
    o = O.Oracle(inp['S'], inp['A'], inp['H'], 'tanh', torch.float64 if fp64 else torch.float32)
    lr = O.lr_vector(o, 0.1, 2, 5)
    return inp, lr, o.meta_lr(inp['theta'], inp['sup'], inp['qry'], [0, 1], lr, [0, 1], kind='a2c')


@pytest.mark.parametrize('T', [1, 3])
def test_odd_parameter_count(T):
    """P = 771: odd, no multiple of 4 or of the block of 256 (four blocks, the last with three live threads); counts below the batch and a
    task with one row.  A2C, second order, per-update rows, against the same fp64 autograd at the bars of the cases above."""
    inp, lr, ref64 = _odd(T, True)
    _, _, ref32 = _odd(T, False)
    eng = PolicyEngine(inp['S'], inp['A'], inp['H'], activation='tanh')
    assert eng.param_count == 771 == inp['theta'].numel()
    theta = _f(inp['theta'])
    got = eng.meta_batch_lr(theta, _batch(inp['sup']), _batch(inp['qry']), [0, 1], _f(lr), [0, 1], loss='a2c')
    torch.cuda.synchronize()
    _check_against(f'odd_771,T={T}', got, inp['theta'], ref64, ref32, T)
    frozen = O.frozen_mask(O.Oracle(inp['S'], inp['A'], inp['H'], 'tanh')).cuda()
    assert torch.equal(got[1][:, frozen], theta[frozen].expand(T, -1))


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('kind,act,epochs,head_only', [('a2c', 'relu', 1, False), ('ppo', 'tanh', 3, False), ('a2c', 'tanh', 1, True)])
def test_update_lr_is_the_forward_half_of_the_fused_call(kind, act, epochs, head_only):
    inp, eng, theta, sup, qry = _setup(act, _algo(kind))
    o = O.Oracle(inp['S'], inp['A'], inp['H'], act)
    lr = _f(O.lr_vector(o, 0.05, 2, 5))
    s0 = {k: v[0] for k, v in sup.items()}
    out, losses = eng.update(theta, s0['states'], s0['actions'], s0['adv'], s0['count'], lr[1], loss=kind, epochs=epochs, clip=0.1,
                             head_only=head_only)
    _, want, _, _ = eng.meta_batch_lr(theta, sup, qry, [0] * epochs, lr, [1] * epochs, loss=kind, clip=0.1, head_only=head_only,
                                      with_grad=False)
    torch.cuda.synchronize()
    assert tuple(losses.shape) == (3, epochs) and torch.equal(out, want) and not torch.equal(out, theta.expand_as(out))
    # from per-task parameters, in place: the rows of the call above once more
    again = out.clone()
    out2, _ = eng.update(again, s0['states'], s0['actions'], s0['adv'], s0['count'], lr[0], loss=kind, epochs=1, clip=0.1, head_only=head_only)
    one, _ = eng.update(again[1:2], s0['states'][1:2], s0['actions'][1:2], s0['adv'][1:2], s0['count'][1:2], lr[0], loss=kind, epochs=1,
                        clip=0.1, head_only=head_only)
    assert torch.equal(out2[1:2], one)


def test_tasks_are_independent_calls_reproducible_and_zero_steps():
    inp, eng, theta, sup, qry = _setup('relu', 'vpg')
    o = O.Oracle(inp['S'], inp['A'], inp['H'], 'relu')
    lr = _f(O.lr_vector(o, 0.05, 2, 5))
    call = lambda s, q: eng.meta_batch_lr(theta, s, q, [0, 1], lr, [0, 1], loss='a2c')
    full = [x.clone() for x in call(sup, qry)]
    for t in range(3):
        l1, th1, _, _ = call({k: v[:, t:t + 1].contiguous() for k, v in sup.items()}, {k: v[t:t + 1].contiguous() for k, v in qry.items()})
        assert torch.equal(l1[0], full[0][t]) and torch.equal(th1[0], full[1][t]), t
    again = call(sup, qry)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, full))
    # steps = 0: the scalar call's loss, theta_out = theta, lr_grad exactly 0
    want = eng.meta_batch(theta, None, qry, [], 0.05, loss='a2c')
    got = eng.meta_batch_lr(theta, None, qry, [], lr, [], loss='a2c')
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert tuple(got[3].shape) == (2, eng.param_count) and torch.equal(got[3], torch.zeros_like(got[3]))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_argument_errors_leave_the_outputs_untouched():
    """MI_ERR_ARG (-1) with the entry's name in the text, before any HIP call: the sentinel-filled outputs keep every bit."""
    inp, eng, theta, sup, qry = _setup('relu', 'vpg')
    T, B, P = 3, qry['states'].shape[1], eng.param_count
    lr = torch.full((2, P), 0.05, device='cuda')
    outs = dict(loss=torch.full((T,), -7.0, device='cuda'), theta=torch.full((T, P), -7.0, device='cuda'),
                grad=torch.full((P,), -7.0, device='cuda'), lr_grad=torch.full((2, P), -7.0, device='cuda'))
    ws = torch.empty(1 << 26, dtype=torch.uint8, device='cuda')
    sb, sn = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 1)

    def call(lr_vec=lr, lr_rows=2, rows=(0, 1), with_grad=1, lr_grad=outs['lr_grad'], steps=2):
        sr = None if rows is None else (C.c_int32 * len(rows))(*rows)
        return eng.lib.mi_policy_meta_batch_lr(
            eng._h, _stream(eng.device), _ptr(theta), steps, sb, sn, sr, 2, _ptr(sup['states']), _ptr(sup['actions']), _ptr(sup['adv']),
            _ptr(sup['count']), None, _ptr(qry['states']), _ptr(qry['actions']), _ptr(qry['adv']), _ptr(qry['count']), None, T, B, 0, 0.1,
            _ptr(lr_vec), lr_rows, 0, 1, with_grad, _ptr(outs['loss']), _ptr(outs['theta']), _ptr(outs['grad']), _ptr(lr_grad), _ptr(ws),
            ws.numel())
    cases = [(dict(lr_vec=None), b'lr_vec'), (dict(lr_rows=0), b'lr_rows 0'), (dict(lr_rows=65536), b'lr_rows 65536'),
             (dict(rows=(0, 2)), b'step_lr_row[1] 2'),
             (dict(rows=(-1, 0)), b'step_lr_row[0] -1'), (dict(with_grad=0), b'lr_grad_out'), (dict(steps=257), b'steps 257')]
    for kw, text in cases:
        assert call(**kw) == -1, kw
        msg = eng.lib.mi_policy_last_error(eng._h)
        assert b'mi_policy_meta_batch_lr' in msg and text in msg, msg
    s0 = {k: v[0] for k, v in sup.items()}

    def upd(lr_vec=lr[0], epochs=1, kind=0):
        return eng.lib.mi_policy_update_lr(eng._h, _stream(eng.device), _ptr(theta), 0, _ptr(s0['states']), _ptr(s0['actions']), _ptr(s0['adv']),
                                           _ptr(s0['count']), None, T, B, kind, epochs, 0.1, _ptr(lr_vec), 0, _ptr(outs['theta']), None,
                                           _ptr(ws), ws.numel())
    for kw, text in ((dict(lr_vec=None), b'lr_vec'), (dict(epochs=0), b'epochs 0'), (dict(kind=2), b'MI_PLOSS_DICE')):
        assert upd(**kw) == -1, kw
        msg = eng.lib.mi_policy_last_error(eng._h)
        assert b'mi_policy_update_lr' in msg and text in msg, msg
    torch.cuda.synchronize()
    assert all(bool((v == -7.0).all()) for v in outs.values())
    assert call() == 0                                                # and the same buffers with nothing wrong: a full call
    torch.cuda.synchronize()
    assert not bool((outs['loss'] == -7.0).any()) and not bool((outs['lr_grad'] == -7.0).any())


# ---------------------------------------------------------------------------------------------------------------- 6
SURFACE = dict(max_path_length=10, adapt_batch_size=4, adapt_steps=2, gamma=0.99, tau=1.0, ppo_epochs=2, ppo_clip_ratio=0.1, inner_lr=0.05)
SEED, FIRST_ID = 31, 1018


def _wrapped(act='tanh'):
    pol = AC.make_policy(act, False, 0.3, True).cuda()
    lr = cf.InnerLR(pol, 0.05, per='tensor', steps=2, learnable=True, frozen=('mean.0.',))
    return pol, lr, cf.MAML(pol, lr=lr)


@pytest.mark.parametrize('algo', ['vpg', 'ppo'])
def test_fast_adapt_tasks_with_a_learnable_inner_lr(algo):
    pol, lr, maml = _wrapped()
    base = cf.LinearValue(2, 2)
    if algo == 'vpg':
        res = cf.fast_adapt_vpg_tasks(AC.GOALS, maml, base, SURFACE, SEED, FIRST_ID)
    else:
        res = cf.fast_adapt_ppo_tasks(AC.GOALS, maml, base, SURFACE, SEED, FIRST_ID)
    res.total_loss.backward()
    for q in list(pol.parameters()) + [lr.values]:
        assert q.grad is not None and bool(torch.isfinite(q.grad).all()) and float(q.grad.abs().max()) > 0
    names = [n for n, _ in pol.named_parameters()]
    assert float(lr.values.grad[:, names.index('mean.0.weight')].abs().max()) == 0          # frozen: no gradient reaches the stored value
    # values.grad = the engine's lr_grad summed per tensor, on the replays the call kept
    eng = pol.engine()
    batches = [cf.rl._replay_batch([task[k] for task in res.replays], 2, 2, pol.sigma.device) for k in range(3)]
    for b in batches:
        b['adv'], _ = cf.rl._batch_advantages(b, cf.LinearValue(2, 2), 0.99, 1.0, normalize=(algo == 'ppo'))
    sup, qry = cf.rl._stack_batches(batches[:2], batches[2])
    epochs = 2 if algo == 'ppo' else 1
    step_batch = [b for b in range(2) for _ in range(epochs)]
    flat = maml.lr_flat().detach().contiguous()
    lt, th, grad, lr_grad = eng.meta_batch_lr(pol.flat(), sup, qry, step_batch, flat, step_batch, loss='ppo' if algo == 'ppo' else 'a2c', clip=0.1)
    assert torch.equal(lt, res.valid_loss) and torch.equal(th, res.theta)
    want, off = torch.zeros_like(lr.values), 0
    for q in pol._engine_params():
        j = [id(x) for x in pol.parameters()].index(id(q))
        if not lr.is_frozen(names[j]):
            want[:, j] = lr_grad[:, off:off + q.numel()].sum(dim=1)
        off += q.numel()
    np.testing.assert_allclose(lr.values.grad.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(torch.cat([q.grad.reshape(-1) for q in pol._engine_params()]).cpu().numpy(), grad.cpu().numpy(), rtol=0, atol=0)
    # the task walk with the same rollout ids: adapted parameters and the summed loss bit for bit
    walk_pol, _, walk = _wrapped()
    base_b, total = cf.LinearValue(2, 2), 0.0
    for i, goal in enumerate(AC.GOALS):
        runner = cf.Particles2DRunner(goal, SURFACE['max_path_length'], rollout='device', seed=SEED, first_id=FIRST_ID + i * 3)
        learner = walk.clone()
        loss, _, _ = (cf.fast_adapt_vpg if algo == 'vpg' else cf.fast_adapt_ppo)(runner, learner, base_b, SURFACE)
        total = total + loss
        assert torch.equal(learner._adapted_policy.flat(), res.theta[i]), i
        assert torch.equal(loss.detach(), res.valid_loss[i]), i
    assert torch.equal(total.detach(), res.total_loss.detach())
    assert not torch.equal(res.theta[:, 2:], pol.flat()[2:].expand(3, -1))
    w1 = slice(2, 2 + 200 + 100)
    assert torch.equal(res.theta[:, w1], pol.flat()[w1].expand(3, -1))                     # mean.0. is frozen


def test_stepwise_learner_reaches_the_fused_theta_1():
    pol, lr, maml = _wrapped()
    base = cf.LinearValue(2, 2)
    runner = cf.Particles2DRunner(AC.GOALS[1], 10, rollout='device', seed=SEED, first_id=FIRST_ID)
    episodes = runner.run(pol, episodes=4)
    learner = maml.clone()
    learner.adapt(cf.rl.vpg_a2c_loss(episodes, learner, base, 0.99, 1.0))
    b = cf.rl._replay_batch([cf.rl._as_replay(episodes)], 2, 2, pol.sigma.device)
    adv, _ = cf.rl._batch_advantages(b, cf.LinearValue(2, 2), 0.99, 1.0, normalize=False)
    want, _ = pol.engine().update(pol.flat(), b['states'], b['actions'], adv, b['count'], maml.lr_flat()[0].detach().contiguous())
    got = learner.fast_weights().detach()
    torch.cuda.synchronize()
    step = rel_err((got - pol.flat()).cpu().numpy(), (want[0] - pol.flat()).cpu().numpy())
    report('policy_lr_stepwise_theta1', theta_rel=rel_err(got.cpu().numpy(), want[0].cpu().numpy()), step_rel=step)
    assert rel_err(got.cpu().numpy(), want[0].cpu().numpy()) <= 1e-5
    assert not torch.equal(got, pol.flat())
    learner.adapt(cf.rl.vpg_a2c_loss(episodes, learner, base, 0.99, 1.0))                     # the second step reads row 1
    assert learner.__dict__['_steps_done'] == 2


def test_driver_learns_the_inner_lr_and_trpo_refuses_it():
    from exploring_meta_amd.rl import maml_ppo
    p = dict(maml_ppo.params, meta_batch_size=3, adapt_batch_size=4, max_path_length=10, adapt_steps=2, ppo_epochs=2, num_iterations=2,
             inner_lr=0.05, inner_lr_per='tensor', learn_inner_lr=True)
    policy = maml_ppo.run(p, log=lambda *a: None, rollout='device', batch_tasks=True)
    assert isinstance(policy.lr, cf.InnerLR) and policy.lr.learnable and tuple(policy.lr.values.shape) == (1, 7)
    v = policy.lr.values.detach()
    assert bool(torch.isfinite(v).all()) and not torch.equal(v, torch.full_like(v, 0.05))
    assert all(bool(torch.isfinite(q).all()) for q in policy.parameters())
    pol, lr, maml = _wrapped()
    with pytest.raises(ValueError, match='meta_optimize_trpo'):
        cf.meta_optimize_trpo(dict(SURFACE), maml, cf.LinearValue(2, 2), [], [])
    runner = cf.Particles2DRunner(AC.GOALS[1], 10, rollout='device', seed=SEED, first_id=FIRST_ID)
    with pytest.raises(ValueError, match='fast_adapt_trpo'):
        cf.fast_adapt_trpo(runner, maml, cf.LinearValue(2, 2), dict(SURFACE))
    with pytest.raises(ValueError, match='adapt_steps'):
        cf.fast_adapt_vpg_tasks(AC.GOALS, maml, cf.LinearValue(2, 2), dict(SURFACE, adapt_steps=3), SEED, FIRST_ID)
