"""The device rollout on the host: the numpy restatement of its noise on hand-made words and against Philox's
counter layout, the argument checks of mi_particles_rollout (they run before any HIP call, so without a device), and the inputs of
tests/test_gpu_rollout.py checked on the fp64 oracle alone.  Replaces (reference) core_functions/runner.py + learn2learn Particles2D."""
import ctypes as C
import math

import numpy as np
import pytest

import rollout_oracle as O
from exploring_meta_amd import _lib
from exploring_meta_amd.utils import rollout_ref as RR
from exploring_meta_amd.utils.task_sampler import philox4x32


# ---------------------------------------------------------------------------------------------------- noise
def test_noise_of_the_extreme_words():
    """w0 = 0xffffffff -> u1 = 1 -> r = 0 -> eps = (0, 0) whatever the angle; w0 = 0 -> u1 = 2^-24, the largest radius
    sqrt(2 * 24 * ln 2) = 5.768..; w1 picks the angle: 0 -> (r, 0), 2^31 -> u2 = 1/2 -> (-r, 0), 2^30 -> u2 = 1/4 -> (0, r)."""
    for w1 in (0, 0x12345678, 0xffffffff):
        assert RR.noise_from_words(0xffffffff, w1) == (0.0, 0.0)
    r = math.sqrt(2 * 24 * math.log(2))
    assert RR.noise_from_words(0, 0) == (r, 0.0)
    assert np.allclose(RR.noise_from_words(0, 1 << 31), (-r, 0.0), rtol=0, atol=1e-15)
    assert np.allclose(RR.noise_from_words(0, 1 << 30), (0.0, r), rtol=0, atol=1e-15)
    # the low 8 bits of either word do not take part
    assert RR.noise_from_words(0xab, 0xcd) == RR.noise_from_words(0, 0)
    # u1 in (0, 1], u2 in [0, 1): |eps| <= r everywhere
    assert all(math.hypot(*RR.noise_from_words(w0, w1)) <= r * (1 + 1e-15) for w0 in (0, 255, 256, 1 << 31) for w1 in (0, 77 << 8, 0xffffff00))


@pytest.mark.parametrize('seed,rid,episode,step', [(0, 0, 0, 0), (42, 7, 3, 99), (2 ** 64 - 1, 2 ** 64 - 1, 255, 999),
                                                   (0x0123456789abcdef, 0xfedcba9876543210, 17, 5)])
def test_noise_counter_layout(seed, rid, episode, step):
    """counter = (id_lo, id_hi, episode, step), key = (seed_lo, seed_hi); the package's restatement and the tests' oracle agree."""
    w = philox4x32((rid & 0xffffffff, rid >> 32, episode, step), (seed & 0xffffffff, seed >> 32))
    assert RR.rollout_noise(seed, rid, episode, step) == RR.noise_from_words(w[0], w[1])
    assert RR.rollout_noise(seed, rid, episode, step) == O.noise(seed, rid, episode, step)


def test_noise_separates_its_four_arguments():
    base = RR.rollout_noise(5, 9, 2, 3)
    assert len({base, RR.rollout_noise(6, 9, 2, 3), RR.rollout_noise(5, 10, 2, 3), RR.rollout_noise(5, 9 + 2 ** 32, 2, 3),
                RR.rollout_noise(5, 9, 3, 3), RR.rollout_noise(5, 9, 2, 4), RR.rollout_noise(5 + 2 ** 32, 9, 2, 3)}) == 7


def test_noise_moments():
    """4096 draws: mean within 5 standard errors of 0, variance within 10 % of 1 (a sanity check of the mapping, not of Philox)."""
    x = np.asarray([RR.rollout_noise(1, 2, e, t) for e in range(64) for t in range(32)]).reshape(-1)
    assert abs(x.mean()) < 5 / math.sqrt(x.size) and abs(x.var() - 1.0) < 0.1


def test_package_rollout_equals_the_oracle():
    """exploring_meta_amd.utils.rollout_ref.rollout and tests/rollout_oracle.rollout were written separately from the contract."""
    theta = O.homing_theta([0.1, -0.2])
    a = RR.rollout(theta, O.HOMING_HIDDENS, 'relu', [0.1, -0.2], 9, 4, 3, 25)
    b = O.rollout(theta, O.HOMING_HIDDENS, 'relu', [0.1, -0.2], 9, 4, 3, 25)
    assert a['ep_len'].tolist() == b['ep_len'].tolist()
    for k in ('states', 'actions', 'next_states', 'rewards', 'dones', 'noise'):
        np.testing.assert_allclose(a[k], b[k], rtol=0, atol=1e-14, err_msg=k)


# ---------------------------------------------------------------------------------------------------- the C ABI's argument checks
def _policy(lib, state=2, action=2, h1=100, h2=100, act=0):
    desc = _lib.MiPolicyDesc(state, action, h1, h2, act)
    h = C.c_void_p()
    assert lib.mi_policy_create(C.byref(desc), 0, C.byref(h)) == 0
    return h


def test_abi_rejects_out_of_domain_arguments_before_any_launch():
    """mi_particles_rollout checks the policy's sizes, episodes, max_path_length and tasks on the host: outside its domain it returns
    MI_ERR_ARG with a text naming the entry point and the value, its scratch size is 0, and no device is touched (this runs without
    one; the pointers are never dereferenced)."""
    lib = _lib.load()
    ptr = C.c_void_p(64)

    def call(h, tasks=1, episodes=2, L=3, tstride=0):
        return lib.mi_particles_rollout(h, None, ptr, tstride, ptr, ptr, 1, tasks, episodes, L, ptr, ptr, ptr, ptr, ptr, ptr, None, None,
                                        ptr, 1 << 30)

    ok = _policy(lib)
    cases = [(_policy(lib, state=3), {}, b'state_size 3'), (_policy(lib, action=3), {}, b'action_size 3'),
             (_policy(lib, h1=129), {}, b'129'), (_policy(lib, h2=129), {}, b'129'),
             (ok, dict(episodes=0), b'episodes 0'), (ok, dict(episodes=257), b'episodes 257'),
             (ok, dict(L=0), b'max_path_length 0'), (ok, dict(L=1001), b'max_path_length 1001'),
             (ok, dict(tasks=0), b'tasks 0'), (ok, dict(tasks=-1), b'tasks -1'), (ok, dict(tstride=5), b'tstride 5')]
    for h, kw, text in cases:
        assert call(h, **kw) == -1, kw                                   # MI_ERR_ARG
        msg = lib.mi_policy_last_error(h)
        assert b'mi_particles_rollout' in msg and text in msg, msg
        if 'tstride' not in kw:
            assert lib.mi_particles_rollout_scratch_bytes(h, kw.get('tasks', 1), kw.get('episodes', 2), kw.get('L', 3)) == 0
    assert lib.mi_particles_rollout_scratch_bytes(None, 1, 2, 3) == 0
    # inside the domain the scratch size is positive and grows with every extent; the limits themselves are inside
    small = lib.mi_particles_rollout_scratch_bytes(ok, 1, 2, 3)
    assert small > 0
    assert lib.mi_particles_rollout_scratch_bytes(ok, 2, 256, 1000) >= 2 * 256 * 1000 * 10 * 4
    assert lib.mi_particles_rollout_scratch_bytes(_policy(lib, h1=128, h2=128, act=1), 1, 1, 1) > 0
    for h in {c[0].value: c[0] for c in cases}.values():             # (each handle once: `ok` serves several cases)
        lib.mi_policy_destroy(h)


# ---------------------------------------------------------------------------------------------------- the inputs of the GPU tests
def test_homing_case_is_ragged_reaches_the_cap_and_ends_early():
    case = O.HOMING
    assert case['episodes'] == 8 and case['L'] == 40 and len(case['goals']) == 3
    rolls = O.homing_rollouts()
    lens = [r['ep_len'] for r in rolls]
    print('homing episode lengths', [l.tolist() for l in lens])
    assert len(set(lens[0].tolist())) >= 3                                # ragged inside one task
    allv = np.concatenate(lens)
    assert (allv == case['L']).any() and (allv < case['L']).any()         # one at the cap, one ends early
    assert len({int(l.sum()) for l in lens}) == 3                         # the tasks' counts differ
    for r, goal in zip(rolls, case['goals']):
        ends = np.flatnonzero(r['dones'] == 1.0)
        assert ends.tolist() == (np.cumsum(r['ep_len']) - 1).tolist()
        # far enough from the 0.01 box's edge that fp32 rounding (1e-7) cannot move an ending: the GPU's lengths must be these
        d = np.abs(r['next_states'] - np.float32(goal).astype(np.float64))
        margin = np.abs(d - 0.01).min()
        print('closest approach of |s - goal| to 0.01:', margin)
        assert margin > 1e-5


def test_constant_cases_end_after_exactly_four_rows_and_one_row():
    case = O.CONSTANT
    for goal, rid, rows in zip(case['goals'], case['ids'], case['rows']):
        r = O.rollout(O.constant_theta(), (3, 5), 'relu', np.float32(goal), case['seed'], rid, case['episodes'], case['L'])
        assert r['ep_len'].tolist() == [rows] * case['episodes']
        assert np.exp(max(-20.0, math.log(1e-6))) == pytest.approx(1e-6)
    # with L = 3 the 4-step policy is cut by the cap in every episode
    r = O.rollout(O.constant_theta(), (3, 5), 'relu', np.float32(case['goals'][0]), case['seed'], case['ids'][0], case['episodes'], 3)
    assert r['ep_len'].tolist() == [3] * case['episodes'] and r['dones'].reshape(-1, 3)[:, -1].tolist() == [1.0] * case['episodes']
