"""numpy restatement of the device rollout (mi_particles_rollout): the action noise and a whole Particles2D rollout
in fp64.  Needs no GPU: it re-derives the noise of any (seed, rollout id, episode, step) exactly as the kernel defines it, and a rollout
up to the fp32 rounding of the kernel's arithmetic."""
import math

import numpy as np

from .task_sampler import philox4x32

_M32 = 0xffffffff
LOG_EPSILON = math.log(1e-6)


def noise_from_words(w0, w1):
    """(eps0, eps1) from the first two words of a Philox block: u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u2 = (w1 >> 8) 2^-24 in [0, 1),
    r = sqrt(-2 ln u1), eps = (r cos 2 pi u2, r sin 2 pi u2)."""
    u1 = ((int(w0) >> 8) + 1) * 2.0 ** -24
    u2 = (int(w1) >> 8) * 2.0 ** -24
    r = math.sqrt(-2.0 * math.log(u1))
    return r * math.cos(2.0 * math.pi * u2), r * math.sin(2.0 * math.pi * u2)


def rollout_noise(seed, rid, episode, step):
    """The noise of one step: Philox4x32-10 with key = seed and counter = (id_lo, id_hi, episode, step)."""
    seed, rid = int(seed) & (2 ** 64 - 1), int(rid) & (2 ** 64 - 1)
    w = philox4x32((rid & _M32, rid >> 32, int(episode), int(step)), (seed & _M32, seed >> 32))
    return noise_from_words(w[0], w[1])


def split_theta(theta, hiddens, state_size=2, action_size=2):
    """The flat parameter vector in the engine's order -> (sigma, W1, b1, W2, b2, W3, b3) as fp64 arrays."""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    h1, h2 = hiddens
    shapes = [(action_size,), (h1, state_size), (h1,), (h2, h1), (h2,), (action_size, h2), (action_size,)]
    out, off = [], 0
    for shp in shapes:
        n = int(np.prod(shp))
        out.append(theta[off:off + n].reshape(shp))
        off += n
    if off != theta.size:
        raise ValueError(f'theta has {theta.size} values, the policy {off}')
    return out


def policy_loc(params, activation, states):
    """loc of the policy density for states [n, 2], fp64."""
    _, w1, b1, w2, b2, w3, b3 = params
    act = np.tanh if activation == 'tanh' else (lambda z: np.maximum(z, 0.0))
    h = act(np.asarray(states, dtype=np.float64) @ w1.T + b1)
    h = act(h @ w2.T + b2)
    return h @ w3.T + b3


def rollout(theta, hiddens, activation, goal, seed, rid, episodes, max_path_length):
    """One task's rollout in fp64: the packed replay {states, actions, next_states [n, 2], rewards, dones [n], noise [n, 2], ep_len [E]}."""
    params = split_theta(theta, hiddens)
    scale = np.exp(np.maximum(params[0], LOG_EPSILON))
    goal = np.asarray(goal, dtype=np.float64).reshape(2)
    S, A, NS, R, D, N, lens = [], [], [], [], [], [], []
    for e in range(episodes):
        s = np.zeros(2)
        for t in range(max_path_length):
            eps = np.asarray(rollout_noise(seed, rid, e, t))
            a = policy_loc(params, activation, s[None])[0] + scale * eps
            ns = s + np.clip(a, -0.1, 0.1)
            d = ns - goal
            done = bool((np.abs(d) < 0.01).all())
            S.append(s); A.append(a); NS.append(ns); R.append(-math.sqrt(float(d @ d))); N.append(eps)
            D.append(1.0 if done or t == max_path_length - 1 else 0.0)
            s = ns
            if done:
                break
        lens.append(t + 1)
    two = lambda x: np.asarray(x, dtype=np.float64).reshape(-1, 2)
    return dict(states=two(S), actions=two(A), next_states=two(NS), rewards=np.asarray(R), dones=np.asarray(D), noise=two(N),
                ep_len=np.asarray(lens, dtype=np.int64))
