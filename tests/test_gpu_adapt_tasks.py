"""mi_policy_update and the batched VPG / DiCE / PPO fast-adapt built on it on the GPU:
1. mi_policy_update against mi_policy_meta_batch (bit-identical from shared parameters), per-task starts against single-row calls,
   head_only, the loss before the first update;
2. fast_adapt_vpg_tasks / fast_adapt_ppo_tasks against the task-by-task walk (fast_adapt_vpg / fast_adapt_ppo with per-task device
   runners): replays bit for bit, losses, parameters, rewards, summed gradient, baseline, slices of the goals.  Walk and batched
   call are ONE implementation (core_functions.rl._adapt_and_validate, the walk with one replay row per call), so this checks that
   its results do not depend on how the tasks are batched; what the walk computed before it became that one-task case is held by
   tests/test_gpu_adapt_walk_parity.py;
3. the same calls against the fp64 oracle (oracle/rl_ref.py replay_vpg / replay_ppo) on the replays they returned;
4. the maml_ppo driver with --batch_tasks, evaluate(rollout='device'), single_ppo_update.
Replaces (reference): the per-task loops of core_functions/rl.py:231-255,267-336 and rl/maml_ppo.py:100-131."""
from copy import deepcopy

import numpy as np
import pytest
import torch

import adapt_tasks_cases as AC
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as RLM
from exploring_meta_amd.engine import gae_advantages
from gpu_utils import rel_err, report
from oracle import rl_ref as RL

pytestmark = pytest.mark.gpu

FIELDS = AC.FIELDS
BODY = slice(2, 2 + 100 * 2 + 100 + 100 * 100 + 100)        # W1, b1, W2, b2 of the 2-100-100-2 policy


# ---------------------------------------------------------------------------------------------------- 1. mi_policy_update
_batches = {}


def _batch(act, normalize):
    """One replay per task (device rollout of the 'ragged' policy: the first task ends an episode early) with its advantages."""
    key = (act, normalize)
    if key not in _batches:
        pol = AC.make_policy(act, False, 0.02, True).cuda()
        out = pol.engine().rollout(pol.flat(), np.asarray(AC.GOALS, dtype=np.float32), [AC.FIRST_ID + 2 * i for i in range(3)], AC.SEED,
                                   AC.EPISODES, AC.PATH)
        adv = gae_advantages(out['states'], out['next_states'], out['rewards'], out['dones'], out['count'], 0.99, 1.0, 2, normalize=normalize)
        _batches[key] = (pol, dict(states=out['states'], actions=out['actions'], adv=adv, count=out['count'], done=out['dones']))
    return _batches[key]


UPDATE_CASES = [('a2c', 1, 'relu', False), ('a2c', 2, 'tanh', True), ('ppo', 3, 'relu', False), ('ppo', 3, 'tanh', True),
                ('dice', 1, 'relu', True), ('dice', 2, 'tanh', False)]


@pytest.mark.parametrize('kind,epochs,act,head_only', UPDATE_CASES)
def test_update_equals_meta_batch_from_shared_parameters(kind, epochs, act, head_only):
    """Both run the same passes in the same order: theta_out bit for bit; loss_out[:, 0] is the loss of a no-update evaluation."""
    pol, b = _batch(act, kind == 'ppo')
    eng, theta, lr = pol.engine(), pol.flat(), 2e-3
    assert b['count'].tolist()[0] < AC.EPISODES * AC.PATH == b['count'].tolist()[1]           # ragged
    out, losses = eng.update(theta, b['states'], b['actions'], b['adv'], b['count'], lr, loss=kind, epochs=epochs, clip=0.1,
                             done=b['done'] if kind == 'dice' else None, head_only=head_only)
    sup = {k: v.unsqueeze(0) for k, v in b.items()}
    _, ref, _ = eng.meta_batch(theta, sup, b, [0] * epochs, lr, loss=kind, clip=0.1, head_only=head_only, with_grad=False)
    assert out.shape == ref.shape == (3, theta.numel()) and losses.shape == (3, epochs)
    assert torch.equal(out, ref)
    assert not torch.equal(out[0], theta) and torch.isfinite(out).all() and torch.isfinite(losses).all()
    l0, _, _ = eng.meta_batch(theta, None, b, [], lr, loss=kind, clip=0.1, with_grad=False)
    print(kind, epochs, act, 'loss before the first update', losses[:, 0].tolist(), l0.tolist())
    np.testing.assert_allclose(losses[:, 0].cpu().numpy(), l0.cpu().numpy(), rtol=1e-6, atol=0)
    if head_only:
        assert torch.equal(out[:, BODY], theta[BODY].expand(3, -1))
        assert not torch.equal(out[:, :2], theta[:2].expand(3, -1))
    # every epoch's loss is the loss of a meta_batch evaluation after e updates (the validation loss of PPO has ratio 1: not comparable)
    if kind != 'ppo':
        for e in range(1, epochs):
            le, _, _ = eng.meta_batch(theta, sup, b, [0] * e, lr, loss=kind, clip=0.1, head_only=head_only, with_grad=False)
            np.testing.assert_allclose(losses[:, e].cpu().numpy(), le.cpu().numpy(), rtol=1e-6, atol=0)


@pytest.mark.parametrize('kind,epochs,act,head_only', [('a2c', 1, 'relu', False), ('ppo', 3, 'tanh', True), ('dice', 2, 'relu', False)])
def test_update_from_per_task_rows_equals_single_row_calls(kind, epochs, act, head_only):
    pol, b = _batch(act, kind == 'ppo')
    eng, lr = pol.engine(), 2e-3
    done = b['done'] if kind == 'dice' else None
    rows, _ = eng.update(pol.flat(), b['states'], b['actions'], b['adv'], b['count'], lr, loss=kind, epochs=1, done=done)   # distinct starts
    assert not torch.equal(rows[0], rows[1])
    out, losses = eng.update(rows, b['states'], b['actions'], b['adv'], b['count'], lr, loss=kind, epochs=epochs, done=done, head_only=head_only)
    for t in range(3):
        one = slice(t, t + 1)
        o1, l1 = eng.update(rows[t].contiguous(), b['states'][one], b['actions'][one], b['adv'][one], b['count'][one], lr, loss=kind,
                            epochs=epochs, done=None if done is None else done[one], head_only=head_only)
        np.testing.assert_allclose(out[t].cpu().numpy(), o1[0].cpu().numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(losses[t].cpu().numpy(), l1[0].cpu().numpy(), rtol=1e-6, atol=0)
    if head_only:
        assert torch.equal(out[:, BODY], rows[:, BODY])
    # updating in place (theta_out = theta, per-task rows) gives the same bytes
    again = rows.clone()
    import ctypes as C
    from exploring_meta_amd.engine import _ptr, _stream
    nb = C.c_size_t()
    eng._check(eng.lib.mi_policy_update_workspace_bytes(eng._h, 3, b['states'].shape[1], C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device='cuda')
    eng._check(eng.lib.mi_policy_update(eng._h, _stream(eng.device), _ptr(again), eng.param_count, _ptr(b['states']), _ptr(b['actions']),
                                        _ptr(b['adv']), _ptr(b['count']), _ptr(done), 3, b['states'].shape[1],
                                        {'a2c': 0, 'ppo': 1, 'dice': 2}[kind], epochs, 0.1, lr, int(head_only), _ptr(again), None,
                                        _ptr(ws), ws.numel()))
    assert torch.equal(again, out)


def test_update_rejects_what_it_cannot_do():
    pol, b = _batch('relu', False)
    eng = pol.engine()
    for kw, text in ((dict(epochs=0), 'epochs 0'), (dict(epochs=65), 'epochs 65')):
        with pytest.raises(Exception, match=text):
            eng.update(pol.flat(), b['states'], b['actions'], b['adv'], b['count'], 1e-3, **kw)
    with pytest.raises(ValueError, match='dice'):
        eng.update(pol.flat(), b['states'], b['actions'], b['adv'], b['count'], 1e-3, loss='dice')
    with pytest.raises(ValueError, match='rows'):
        eng.update(pol.flat().expand(2, -1), b['states'], b['actions'], b['adv'], b['count'], 1e-3)


# ---------------------------------------------------------------------------------------------------- 2. against the walk
_results = {}


def _call(name, regime, goals=AC.GOALS, first_id=AC.FIRST_ID, want_replays=True):
    algo, act, anil, first_order, dice, steps, _ = AC.CASES[name]
    pol = AC.case_policy(name, regime).cuda()
    base = cf.LinearValue(2, 2)
    P = AC.case_params(name, regime)
    if algo == 'vpg':
        res = cf.fast_adapt_vpg_tasks(goals, pol, base, P, AC.SEED, first_id, anil=anil, first_order=first_order, dice=dice,
                                      want_replays=want_replays)
    else:
        res = cf.fast_adapt_ppo_tasks(goals, pol, base, P, AC.SEED, first_id, anil=anil, want_replays=want_replays)
    return pol, base, P, res


def _batched(name, regime):
    """One batched call per (case, regime), with its summed gradient, shared by the tests below."""
    key = (name, regime)
    if key not in _results:
        pol, base, P, res = _call(name, regime)
        assert res.total_loss.dim() == 0 and res.valid_loss.shape == res.reward.shape == res.success.shape == (3,)
        res.total_loss.backward()
        grad = torch.cat([q.grad.reshape(-1) for q in pol._engine_params()]).cpu().numpy()
        _results[key] = (pol, base, P, res, grad)
    return _results[key]


@pytest.mark.parametrize('name', list(AC.CASES))
def test_batched_equals_the_task_by_task_walk(name):
    """Replays bit-identical; valid_loss and adapted parameters to rtol 1e-5 (the bar of fast_adapt_trpo_tasks: only the batching
    differs); rewards to 1e-6 relative; summed gradient rel_err <= 1e-5; the baseline ends with the same weights."""
    algo, act, anil, first_order, dice, steps, _ = AC.CASES[name]
    pol, base_a, P, res, grad = _batched(name, 'ragged')
    walk_pol = AC.case_policy(name, 'ragged').cuda()
    assert torch.equal(walk_pol.flat(), pol.flat())
    base_b = cf.LinearValue(2, 2)
    total, counts = 0.0, []
    for i, goal in enumerate(AC.GOALS):
        runner = _Recorder(cf.Particles2DRunner(goal, AC.PATH, rollout='device', seed=AC.SEED, first_id=AC.FIRST_ID + i * (steps + 1)))
        learner = cf.MAML(walk_pol, lr=P['inner_lr'])
        if algo == 'vpg':
            loss, rew, suc = cf.fast_adapt_vpg(runner, learner, base_b, P, anil=anil, first_order=first_order, dice=dice)
        else:
            loss, rew, suc = cf.fast_adapt_ppo(runner, learner, base_b, P, anil=anil)
        total = total + loss
        assert len(runner.replays) == len(res.replays[i]) == steps + 1
        for k_run, (a, b) in enumerate(zip(res.replays[i], runner.replays)):
            for k in FIELDS:
                assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (i, k_run, k)
        counts.append([int(r['states'].shape[0]) for r in runner.replays])
        ta, tb = res.theta[i].cpu().numpy(), learner._adapted_policy.flat().cpu().numpy()
        print(f'{name} task {i}: rows {counts[-1]}, max |dtheta| {np.abs(ta - tb).max():.2e}, loss {float(res.valid_loss[i]):.9g} / '
              f'{float(loss):.9g}, reward {float(res.reward[i]):.7f} / {rew:.7f}')
        np.testing.assert_allclose(ta, tb, rtol=1e-5, atol=0)
        np.testing.assert_allclose(float(res.valid_loss[i]), float(loss), rtol=1e-5, atol=0)
        assert abs(float(res.reward[i]) - rew) <= 1e-6 * abs(rew) and float(res.success[i]) == suc
        assert not np.array_equal(ta, pol.flat().cpu().numpy())
    total.backward()
    gw = torch.cat([q.grad.reshape(-1) for q in walk_pol._engine_params()]).cpu().numpy()
    e_g = rel_err(grad, gw)
    report(f'adapt_tasks_vs_walk[{name}]', grad_rel=e_g, rows=str(counts))
    assert e_g <= 1e-5
    np.testing.assert_allclose(float(res.total_loss), float(total), rtol=1e-5, atol=1e-9)
    np.testing.assert_array_equal(base_a.weight, base_b.weight)
    if not AC.CASES[name][6]:
        assert counts[0][0] < AC.EPISODES * AC.PATH and len({c[0] for c in counts}) > 1     # ragged: the first task ends an episode early
    if anil:
        assert torch.equal(res.theta[:, BODY], pol.flat()[BODY].expand(3, -1))


class _Recorder:
    """A runner that keeps the replays it handed out."""

    def __init__(self, runner):
        self.runner, self.replays = runner, []

    def run(self, policy, episodes):
        self.replays.append(self.runner.run(policy, episodes))
        return self.replays[-1]


@pytest.mark.parametrize('name', ['vpg-tanh-2', 'ppo-relu-1'])
def test_a_slice_of_the_goals_equals_its_rows_of_the_full_call(name):
    """goals[lo:hi] with first_id + lo * (adapt_steps + 1): the replays of rows lo:hi bit for bit (what a rank of the driver computes);
    without replays the same losses, and no read-back of the counts."""
    steps = AC.CASES[name][5]
    _, _, _, full, _ = _batched(name, 'ragged')
    lo, hi = 1, 3
    _, _, _, part = _call(name, 'ragged', AC.GOALS[lo:hi], AC.FIRST_ID + lo * (steps + 1))
    assert len(part.replays) == hi - lo
    for a_task, b_task in zip(part.replays, full.replays[lo:hi]):
        for a, b in zip(a_task, b_task):
            assert all(torch.equal(a[k], b[k]) for k in FIELDS)
    np.testing.assert_allclose(part.valid_loss.cpu().numpy(), full.valid_loss[lo:hi].cpu().numpy(), rtol=1e-5, atol=0)
    _, _, _, bare = _call(name, 'ragged', want_replays=False)
    assert bare.replays is None and torch.equal(bare.valid_loss, full.valid_loss) and torch.equal(bare.theta, full.theta)


# ---------------------------------------------------------------------------------------------------- 3. against the fp64 oracle
@pytest.mark.parametrize('name', list(AC.CASES))
def test_batched_matches_the_fp64_oracle(name):
    """RL.replay_vpg / RL.replay_ppo on the replays the call returned; the bars of test_policy_meta_batch_vpg_ppo: loss 2e-6 of
    max(1, |loss|), parameter step 1e-4, gradient 2e-4."""
    pol, _, P, res, grad = _batched(name, 'smooth')
    leaves = AC.oracle_leaves(pol)
    losses, thetas, gsum = AC.oracle_walk(name, 'smooth', leaves, res.replays)
    theta0 = torch.cat([v.detach().reshape(-1) for v in leaves.values()]).numpy()
    got = res.theta.cpu().numpy().astype(np.float64)
    e_th = max(rel_err(got[t] - theta0, thetas[t] - theta0) for t in range(3))
    e_g = rel_err(grad, gsum)
    e_l = max(abs(float(res.valid_loss[t]) - losses[t]) for t in range(3))
    rows = [[int(r['states'].shape[0]) for r in task] for task in res.replays]
    report(f'adapt_tasks_vs_oracle[{name}]', loss_abs=e_l, theta_step_rel=e_th, grad_rel=e_g, rows=str(rows))
    assert e_l < 2e-6 * max(1.0, max(abs(x) for x in losses))
    assert e_th < 1e-4 and e_g < 2e-4
    if AC.CASES[name][6]:                                                  # the clip is active: after one update some ratios have left the band
        ep = AC.replay64(res.replays[0][0])
        adv = RL.normalize(RL.compute_advantages(RL.LinearValue(2, 2), P['tau'], P['gamma'], ep)).detach()
        old = RL.policy_log_prob(leaves, ep['states'], ep['actions']).detach()
        p1 = RL.maml_adapt_policy(RL.ppo_policy_loss(RL.policy_log_prob(leaves, ep['states'], ep['actions']), old, adv, P['ppo_clip_ratio']),
                                  leaves, P['inner_lr'], True)
        ratio = torch.exp(RL.policy_log_prob(p1, ep['states'], ep['actions']) - old)
        out = int(((ratio < 1 - P['ppo_clip_ratio']) | (ratio > 1 + P['ppo_clip_ratio'])).sum())
        print('ratios outside the clip band after the first epoch:', out, 'of', ratio.numel())
        assert 0 < out


# ---------------------------------------------------------------------------------------------------- 4. driver, evaluate, single update
def _driver(batch_tasks, iterations=2):
    from exploring_meta_amd.rl import maml_ppo
    p = dict(maml_ppo.params, num_iterations=iterations, meta_batch_size=3, adapt_batch_size=4, max_path_length=12, seed=13)
    lines = []
    policy = maml_ppo.run(p, log=lines.append, rollout='device', batch_tasks=batch_tasks)
    assert len(lines) == iterations and torch.isfinite(policy.flat()).all()
    assert all('nan' not in ln and 'inf' not in ln for ln in lines), lines
    return lines


def test_maml_ppo_driver_with_batched_tasks():
    a, b = _driver(True), _driver(True)
    print(a)
    assert a == b                                                          # reproducible
    walk = _driver(False, iterations=1)
    num = lambda ln: [float(x) for x in (ln.split()[3], ln.split()[5])]
    print(walk[0], '|', a[0])
    np.testing.assert_allclose(num(a[0]), num(walk[0]), rtol=1e-4, atol=0)


@pytest.mark.parametrize('algo,anil', [('vpg', False), ('vpg', True), ('ppo', False)])
def test_evaluate_on_device_equals_per_task_device_runners(algo, anil):
    K = 2
    P = dict(AC.PARAMS, inner_lr=2e-3, adapt_steps=K, seed=7, n_tasks=3)
    pol = AC.make_policy('tanh', anil, 0.02, True).cuda()
    before = pol.flat().clone()
    base_a, base_b = cf.LinearValue(2, 2), cf.LinearValue(2, 2)
    rewards, mean_rew, mean_suc = RLM.evaluate(algo, None, pol, base_a, P, anil=anil, goals=AC.GOALS, rollout='device', first_id=50)
    assert torch.equal(pol.flat(), before) and len(rewards) == 3 and mean_suc == 0.0
    want = []
    for i, goal in enumerate(AC.GOALS):
        runner = cf.Particles2DRunner(goal, AC.PATH, rollout='device', seed=7, first_id=50 + i * (K + 2))
        learner = deepcopy(pol)
        with torch.no_grad():
            if algo == 'vpg':
                cf.fast_adapt_vpg(runner, learner, base_b, P, anil=anil)
            else:
                cf.fast_adapt_ppo(runner, learner, base_b, P)
        query = runner.run(learner._adapted_policy, AC.EPISODES)
        want.append(query['rewards'].sum().item() / AC.EPISODES)
    print(algo, anil, rewards, want)
    np.testing.assert_allclose(rewards, want, rtol=1e-6, atol=0)
    assert mean_rew == pytest.approx(sum(want) / 3, rel=1e-6)
    np.testing.assert_array_equal(base_a.weight, base_b.weight)
    with pytest.raises(NotImplementedError):
        RLM.evaluate('trpo', None, pol, base_a, P, goals=AC.GOALS, rollout='device')


@pytest.mark.parametrize('act,anil', [('relu', False), ('tanh', True)])
def test_single_ppo_update_matches_one_oracle_step(act, anil):
    P = dict(AC.PARAMS, inner_lr=0.05)
    pol = AC.make_policy(act, anil, 0.3, True).cuda()
    replay = cf.Particles2DRunner(AC.GOALS[1], AC.PATH, rollout='device', seed=AC.SEED, first_id=5).run(pol, AC.EPISODES)
    leaves = AC.oracle_leaves(pol)
    ep = AC.replay64(replay)
    activation = torch.relu if act == 'relu' else torch.tanh
    adv = RL.normalize(RL.compute_advantages(RL.LinearValue(2, 2), P['tau'], P['gamma'], ep)).detach()
    with torch.no_grad():
        old = RL.policy_log_prob(leaves, ep['states'], ep['actions'], activation)
    new = RL.policy_log_prob(RL._body_detached(leaves, anil), ep['states'], ep['actions'], activation)
    loss64 = RL.ppo_policy_loss(new, old, adv, P['ppo_clip_ratio'])
    p64 = RL.maml_adapt_policy(loss64, leaves, P['inner_lr'], True, head_only=anil)
    theta0 = pol.flat().clone()
    if anil:
        pol.turn_off_body_grads()
    learner = cf.MAML(pol, lr=P['inner_lr'])
    loss = cf.single_ppo_update(replay, learner, cf.LinearValue(2, 2), P, anil=anil)
    t0 = theta0.cpu().numpy().astype(np.float64)
    step = pol.flat().cpu().numpy().astype(np.float64) - t0
    want = torch.cat([v.detach().reshape(-1) for v in p64.values()]).numpy() - t0
    e_th, e_l = rel_err(step, want), abs(float(loss) - float(loss64))
    report(f'single_ppo_update[{act},anil={anil}]', loss_abs=e_l, theta_step_rel=e_th)
    assert e_l < 2e-6 * max(1.0, abs(float(loss64))) and e_th < 1e-4
    assert np.linalg.norm(step) > 0
    if anil:
        assert torch.equal(pol.flat()[BODY], theta0[BODY])
