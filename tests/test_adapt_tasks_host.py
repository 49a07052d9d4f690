"""The batched VPG / DiCE / PPO fast-adapt on the host: the new symbols are declared and exported, the argument
checks of mi_policy_update (they run before any HIP call, so without a device), the rollout-id arithmetic of the batched calls under
every rank split, the driver's refusal of --batch_tasks without device rollouts, and the inputs of tests/test_gpu_adapt_tasks.py
checked on the fp64 restatement of the rollout.  Replaces (reference): the per-task loops of core_functions/rl.py:231-255,267-336."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adapt_tasks_cases as AC
from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as RLM
from exploring_meta_amd.sharding import shard_range
from exploring_meta_amd.utils import rollout_ref as RR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_symbols_are_declared_and_exported():
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    lib = _lib.load()
    for name in ('mi_policy_update', 'mi_policy_update_workspace_bytes'):
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.EXPORTS and getattr(lib, name) is not None
    for name in ('fast_adapt_vpg_tasks', 'fast_adapt_ppo_tasks', 'single_ppo_update'):
        assert callable(getattr(cf, name)) and getattr(cf, name) is getattr(RLM, name)
    from exploring_meta_amd.engine import PolicyEngine
    assert callable(PolicyEngine.update)
    import inspect
    assert 'rollout' in inspect.signature(RLM.evaluate).parameters
    from exploring_meta_amd.rl import maml_ppo
    assert inspect.signature(maml_ppo.run).parameters['batch_tasks'].default is False


def _policy(lib):
    desc = _lib.MiPolicyDesc(2, 2, 100, 100, 0)
    h = C.c_void_p()
    assert lib.mi_policy_create(C.byref(desc), 0, C.byref(h)) == 0
    return h


def test_update_rejects_out_of_domain_arguments_before_any_launch():
    """MI_ERR_ARG with a text naming mi_policy_update and the value; no device is touched (this runs without one; the pointers are
    never dereferenced)."""
    lib = _lib.load()
    ptr = C.c_void_p(64)

    def call(h, tasks=1, batch=4, kind=0, epochs=1, tstride=0, done=None, theta_out=None):
        return lib.mi_policy_update(h, None, ptr, tstride, ptr, ptr, ptr, ptr, done, tasks, batch, kind, epochs, 0.1, 0.1, 0,
                                    theta_out or C.c_void_p(128), ptr, ptr, 1 << 30)

    assert call(None) == -1 and b'mi_policy_update' in lib.mi_policy_last_error(None) and b'null' in lib.mi_policy_last_error(None)
    h = _policy(lib)
    cases = [(dict(epochs=0), b'epochs 0'), (dict(epochs=65), b'epochs 65'), (dict(epochs=-3), b'epochs -3'), (dict(kind=2), b'MI_PLOSS_DICE'),
             (dict(kind=3), b'loss_kind 3'), (dict(tasks=0), b'tasks 0'), (dict(batch=0), b'batch 0'), (dict(tstride=5), b'tstride 5'),
             (dict(tasks=2, theta_out=ptr), b'alias')]
    for kw, text in cases:
        assert call(h, **kw) == -1, kw                                     # MI_ERR_ARG
        msg = lib.mi_policy_last_error(h)
        assert b'mi_policy_update' in msg and text in msg, msg
    n = C.c_size_t()
    assert lib.mi_policy_update_workspace_bytes(None, 1, 4, C.byref(n)) == -1
    assert lib.mi_policy_update_workspace_bytes(h, 0, 4, C.byref(n)) == -1
    assert lib.mi_policy_update_workspace_bytes(h, 1, 4, C.byref(n)) == 0 and n.value > 0
    small = n.value
    assert lib.mi_policy_update_workspace_bytes(h, 3, 48, C.byref(n)) == 0 and n.value > small
    lib.mi_policy_destroy(h)


@pytest.mark.parametrize('T,steps', [(1, 1), (3, 2), (20, 1), (20, 3), (7, 0)])
def test_rollout_ids_of_the_rank_slices_are_those_of_the_task_loop(T, steps):
    """Whatever the world size, rank r's batched call over goals[lo:hi] with first_id (it * T + lo) * runs gives task g the ids
    (it * T + g) * runs + k of the driver's task loop: disjoint over tasks and iterations, and a partition of the loop's ids."""
    runs = steps + 1
    for it in (0, 1, 5):
        loop = {g: [(it * T + g) * runs + k for k in range(runs)] for g in range(T)}
        for world in range(1, T + 2):
            got = {}
            for rank in range(world):
                lo, hi = shard_range(T, rank, world)
                if hi == lo:
                    continue
                ids = RLM._task_rollout_ids((it * T + lo) * runs, hi - lo, steps)
                assert len(ids) == runs and all(len(row) == hi - lo for row in ids)
                for i, g in enumerate(range(lo, hi)):
                    assert g not in got
                    got[g] = [ids[k][i] for k in range(runs)]
            assert got == loop, (it, world)
        flat = [x for v in loop.values() for x in v]
        assert len(set(flat)) == len(flat) and min(flat) == it * T * runs and max(flat) == (it + 1) * T * runs - 1
    # a caller that reserves further runs per task (evaluate: the final episodes) widens the stride
    assert RLM._task_rollout_ids(50, 3, 2, stride=4) == [[50, 54, 58], [51, 55, 59], [52, 56, 60]]


def test_batch_tasks_needs_device_rollouts():
    from exploring_meta_amd.rl import maml_ppo
    for rollout in (None, 'host'):
        with pytest.raises(ValueError, match='batch_tasks'):
            maml_ppo.run(dict(maml_ppo.params), rollout=rollout, batch_tasks=True)
    r = subprocess.run([sys.executable, '-m', 'exploring_meta_amd.rl.maml_ppo', '--batch_tasks'], cwd=REPO, capture_output=True, text=True)
    assert r.returncode == 2 and '--batch_tasks needs --rollout device' in r.stderr


def test_batched_calls_refuse_replays_the_advantage_kernel_cannot_hold(monkeypatch):
    pol = AC.make_policy('relu', False, 0.3, False)
    monkeypatch.setattr(RLM, '_gae_on_device', lambda dev, S, rows: False)
    monkeypatch.setattr(RLM, '_gae_max_rows', lambda S: 2048)
    monkeypatch.setattr(type(pol), 'engine', lambda self: None)
    P = dict(AC.PARAMS, inner_lr=0.1, adapt_steps=1)
    with pytest.raises(ValueError, match='fast_adapt_vpg_tasks keeps replays of 4 x 12 rows'):
        cf.fast_adapt_vpg_tasks(AC.GOALS, pol, cf.LinearValue(2, 2), P, 0, 0)
    with pytest.raises(ValueError, match='fast_adapt_ppo_tasks'):
        cf.fast_adapt_ppo_tasks(AC.GOALS, pol, cf.LinearValue(2, 2), P, 0, 0)


def test_the_ragged_policies_end_an_episode_of_the_first_task_early():
    """Run 0 of the first goal under FIRST_ID on the fp64 restatement of the rollout: fewer rows than episodes x path for the relu, tanh
    and ANIL policies, every |s - goal| far enough from the 0.01 box's edge that fp32 rounding (1e-7) cannot move an ending; the
    other goals are out of reach."""
    full = AC.EPISODES * AC.PATH
    for act, anil in (('relu', False), ('tanh', False), ('tanh', True)):
        pol = AC.make_policy(act, anil, *AC.REGIMES['ragged'][::2])
        theta = torch.cat([q.detach().reshape(-1) for q in pol._engine_params()]).double().numpy()
        rows = []
        for goal in AC.GOALS:
            r = RR.rollout(theta, (100, 100), act, np.float32(goal), AC.SEED, AC.FIRST_ID, AC.EPISODES, AC.PATH)
            d = np.abs(np.asarray(r['next_states']) - np.float32(goal).astype(np.float64))
            assert np.abs(d.max(axis=1) - 0.01).min() > 1e-4              # done = both |s - goal| < 0.01, i.e. the larger one
            rows.append(len(r['rewards']))
        print(act, anil, rows)
        assert rows[0] < full and rows[1] == rows[2] == full
