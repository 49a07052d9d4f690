"""fp64 numpy oracle of a Particles2D rollout as mi_particles_rollout defines it, written from the contract:

  noise   Philox4x32-10, key = seed, counter = (id_lo, id_hi, episode, step); u1 = ((w0 >> 8) + 1) 2^-24, u2 = (w1 >> 8) 2^-24,
          r = sqrt(-2 ln u1), eps = (r cos 2 pi u2, r sin 2 pi u2)
  policy  theta = (sigma[2], W1[H1,2], b1, W2[H2,H1], b2, W3[2,H2], b3); loc = W3 act(W2 act(W1 s + b1) + b2) + b3,
          scale = exp(max(sigma, log 1e-6)); a = loc + scale * eps (stored unclipped)
  env     s_0 = 0, s' = s + clip(a, +-0.1), reward = -|s' - goal|_2, done = both |s' - goal| < 0.01; an episode's rows are steps
          0 .. t_done (or L - 1), the stored done flag is 1 on its last row only

and the hand-made policies and committed seeds of tests/test_rollout_host.py / tests/test_gpu_rollout.py."""
import math

import numpy as np

from exploring_meta_amd.utils.task_sampler import philox4x32

M32 = 0xffffffff


def words_to_noise(w0, w1):
    u1 = ((w0 >> 8) + 1) / 16777216.0
    u2 = (w1 >> 8) / 16777216.0
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


def noise(seed, rid, episode, step):
    w = philox4x32((rid & M32, (rid >> 32) & M32, episode, step), (seed & M32, (seed >> 32) & M32))
    return words_to_noise(w[0], w[1])


def split(theta, hiddens):
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    h1, h2 = hiddens
    out, off = [], 0
    for shp in [(2,), (h1, 2), (h1,), (h2, h1), (h2,), (2, h2), (2,)]:
        n = int(np.prod(shp))
        out.append(theta[off:off + n].reshape(shp))
        off += n
    assert off == theta.size, (off, theta.size)
    return out


def join(sigma, w1, b1, w2, b2, w3, b3):
    return np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in (sigma, w1, b1, w2, b2, w3, b3)])


def loc_scale(theta, hiddens, activation, states):
    """(loc [n, 2], scale [2]) in fp64 for states [n, 2]."""
    sigma, w1, b1, w2, b2, w3, b3 = split(theta, hiddens)
    act = np.tanh if activation == 'tanh' else (lambda z: np.maximum(z, 0.0))
    h = act(np.asarray(states, dtype=np.float64).reshape(-1, 2) @ w1.T + b1)
    h = act(h @ w2.T + b2)
    return h @ w3.T + b3, np.exp(np.maximum(sigma, math.log(1e-6)))


def rollout(theta, hiddens, activation, goal, seed, rid, episodes, L):
    """One task in fp64 -> dict of the packed rows (states, actions, next_states [n, 2], rewards, dones [n], noise [n, 2]) and
    ep_len [episodes]."""
    goal = np.asarray(goal, dtype=np.float64).reshape(2)
    rows = {k: [] for k in ('states', 'actions', 'next_states', 'rewards', 'dones', 'noise')}
    lens = []
    for e in range(episodes):
        s = np.zeros(2)
        for t in range(L):
            eps = np.asarray(noise(seed, rid, e, t))
            loc, scale = loc_scale(theta, hiddens, activation, s)
            a = loc[0] + scale * eps
            ns = s + np.clip(a, -0.1, 0.1)
            d = ns - goal
            done = abs(d[0]) < 0.01 and abs(d[1]) < 0.01
            for k, v in (('states', s), ('actions', a), ('next_states', ns), ('rewards', -math.sqrt(d[0] * d[0] + d[1] * d[1])),
                         ('dones', 1.0 if (done or t == L - 1) else 0.0), ('noise', eps)):
                rows[k].append(v)
            s = ns
            if done:
                break
        lens.append(t + 1)
    out = {k: np.asarray(v, dtype=np.float64) for k, v in rows.items()}
    out['ep_len'] = np.asarray(lens, dtype=np.int64)
    return out


# ---------------------------------------------------------------------------------------------------- hand-made policies
HOMING_HIDDENS = (4, 4)


def homing_theta(goal, c=0.5, sigma=math.log(0.02)):
    """h1 = relu(W1 s) = (x+, x-, y+, y-), W2 = identity, loc = c (goal - s): the goal sits in b3, so every task has its own theta.
    With noise of scale 0.02 around a contraction by 1 - c the episodes end at random times."""
    goal = np.asarray(goal, dtype=np.float64).reshape(2)
    w1 = np.array([[1, 0], [-1, 0], [0, 1], [0, -1]], dtype=np.float64)
    w3 = np.array([[-c, c, 0, 0], [0, 0, -c, c]], dtype=np.float64)
    return join([sigma, sigma], w1, np.zeros(4), np.eye(4), np.zeros(4), w3, c * goal)


def constant_theta(hiddens=(3, 5)):
    """All weights zero, b3 = (0.05, 0.05), sigma = -20 (clamped to log 1e-6): every step moves by (0.05, 0.05) + 1e-6 eps."""
    h1, h2 = hiddens
    return join([-20.0, -20.0], np.zeros((h1, 2)), np.zeros(h1), np.zeros((h2, h1)), np.zeros(h2), np.zeros((2, h2)), [0.05, 0.05])


def default_theta(hiddens, activation, seed):
    """A default-initialised DiagNormalPolicy (xavier-uniform weights, zero biases, sigma = 0) with non-zero biases and sigma = log 0.3
    put in, so that every parameter group takes part."""
    import torch
    from exploring_meta_amd.core_functions import DiagNormalPolicy
    torch.manual_seed(seed)
    pol = DiagNormalPolicy(2, 2, list(hiddens), activation=activation)
    theta = pol.flat().numpy().copy()
    rng = np.random.default_rng(seed)
    sigma, w1, b1, w2, b2, w3, b3 = split(theta, hiddens)
    return join(np.log([0.3, 0.2]), w1, rng.uniform(-0.1, 0.1, b1.shape), w2, rng.uniform(-0.1, 0.1, b2.shape), w3,
                rng.uniform(-0.05, 0.05, b3.shape))


# ---------------------------------------------------------------------------------------------------- committed cases
# The homing case of the GPU tests: 3 tasks x 8 episodes, L = 40.  The seed was searched on this oracle (tests/test_rollout_host.py states
# the conditions): task 0 has at least 3 distinct episode lengths, at least one episode of the case runs to the cap, at least one ends early,
# and the tasks' counts differ.
HOMING = dict(seed=4, ids=[11, 2 ** 40 + 5, 2 ** 63 + 9], goals=[[0.31, -0.22], [-0.12, 0.4], [0.05, 0.07]], episodes=8, L=40)
# The constant cases: goal (0.2, 0.2) ends every episode after exactly 4 rows, goal (0.05, 0.05) after exactly 1.
CONSTANT = dict(seed=7, ids=[3, 4], goals=[[0.2, 0.2], [0.05, 0.05]], rows=[4, 1], episodes=5, L=9)


def homing_rollouts(case=None):
    case = case or HOMING
    return [rollout(homing_theta(g), HOMING_HIDDENS, 'relu', np.float32(g), case['seed'], rid, case['episodes'], case['L'])
            for g, rid in zip(case['goals'], case['ids'])]
