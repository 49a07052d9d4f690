"""MAML-TRPO functions with the reference's names (core_functions/rl.py TRPO part, lines 95-110 and 346-473) on the batched
HIP policy engine.  Replays are either dicts of tensors ``states [N,S], actions [N,A], rewards [N,1], dones [N,1], next_states
[N,S]`` (episodes concatenated; what this package's runners return) or any object with cherry ExperienceReplay's accessors
``state() action() reward() done() next_state()`` (+ ``success()`` where the runner records it) -- what the reference's own call
sites pass (rl.py:49-56, rl/maml_trpo.py:106-134); ``_as_replay`` reads either.
Host side (tiny): discounting, the LinearValue least-squares baseline, GAE, normalisation.
Device side: policy forward, the inner ``trpo_update``, the meta surrogate loss / KL, its gradient, and the Fisher-vector
products inside conjugate gradient -- for ALL tasks of the meta-batch per call.
"""
from copy import deepcopy

import numpy as np
import torch

device = torch.device('cuda')


def set_device(dev):
    """reference rl.py:44-46"""
    global device
    device = dev


# ---------------------------------------------------------------------------------------------- replays
_ACCESSORS = (('states', 'state'), ('actions', 'action'), ('rewards', 'reward'), ('dones', 'done'), ('next_states', 'next_state'))


def _as_replay(episodes):
    """A replay as the dict the rest of this module reads.  Dicts pass through; an object with cherry ExperienceReplay's accessors
    (reference rl.py:49-56 ``get_episode_values``: ``state() action() reward() done() next_state()``) is read ONCE into a ``Replay``
    that is remembered on the object (``_mi_replay``), so the meta-step that walks the same replays again (rl.py:444-465) finds the same
    tensors -- and the device addresses already checked for them.  ``success()`` (rl.py:59-72), where present, rides along."""
    if isinstance(episodes, dict):
        return episodes
    memo = getattr(episodes, '_mi_replay', None)
    if memo is not None:
        return memo
    try:
        fields = {k: getattr(episodes, a)() for k, a in _ACCESSORS}
    except AttributeError as e:
        raise TypeError(f'a replay must be a dict of tensors or offer state() / action() / reward() / done() / next_state(): {e}') from None
    n = fields['states'].shape[0]
    fields['rewards'], fields['dones'] = fields['rewards'].reshape(n, 1), fields['dones'].reshape(n, 1)
    suc = getattr(episodes, 'success', None)
    if callable(suc):
        fields['success'] = suc()
    out = Replay(fields)
    try:
        episodes._mi_replay = out
    except Exception:                                      # (objects without a __dict__: converted again next time)
        pass
    return out


_warned_no_success = [False]


def get_ep_successes(episodes, path_length):
    """reference rl.py:59-72: the number of rows of ``success`` reshaped (path_length, -1).T that hold at least one success flag.
    The reference's runner flattens its replay episode by episode (runner.py ``flatten_episodes``), so that reshape does NOT put
    one episode per row: row j collects the steps j, j + episodes, j + 2 episodes, ... of the flat replay.  This is a quirk of
    the reference, reproduced here as it is (an all-success episode 0 next to an episode 1 without any counts 2).  Without a
    success record the reference prints 'No success metric registered!' and counts 0 -- here the notice is printed once per process."""
    suc = _as_replay(episodes).get('success')
    if suc is None:
        if not _warned_no_success[0]:
            _warned_no_success[0] = True
            print('No success metric registered!')
        return 0
    suc = torch.as_tensor(suc).detach().reshape(path_length, -1).T
    return int((suc == 1.).any(dim=1).sum().item())


# ---------------------------------------------------------------------------------------------- host-side pieces (cherry semantics)
def _np(x):
    return x.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(x) else np.asarray(x, dtype=np.float64)


def discount(gamma, rewards, dones):
    """cherry.td.discount: R_t = r_t + gamma (1 - d_t) R_{t+1}.  A `done` cuts the recursion, so the replay splits into episodes;
    they are padded with zeros at the END to a common length (zeros behind the last step leave the backward recursion at exactly
    0) and the whole replay is one linear-filter call along the time axis -- bit-identical to the step-by-step loop."""
    try:
        from scipy.signal import lfilter
    except ImportError:                                    # scipy is optional (not in the reference's requirements): plain recursion
        lfilter = None
    r = rewards[:, 0]
    n = r.shape[0]
    ends = np.flatnonzero(dones[:, 0] != 0.0)
    if ends.size == 0 or ends[-1] != n - 1:
        ends = np.append(ends, n - 1)
    starts = np.concatenate([[0], ends[:-1] + 1])
    lens = ends - starts + 1
    L = int(lens.max())
    ep = np.repeat(np.arange(lens.size), lens)             # episode of every step
    pos = np.arange(n) - starts[ep]                        # position inside its episode
    pad = np.zeros((lens.size, L))
    pad[ep, pos] = r
    if lfilter is not None:
        disc = lfilter([1.0], [1.0, -gamma], pad[:, ::-1], axis=1)[:, ::-1]
    else:
        disc = pad.copy()
        for i in range(L - 2, -1, -1):
            disc[:, i] = pad[:, i] + gamma * disc[:, i + 1]
    out = np.empty_like(rewards)
    out[:, 0] = disc[ep, pos]
    return out


class LinearValue:
    """cherry.models.robotics.LinearValue(input_size, reg): features [s, s^2, t, t^2, t^3, 1], t = arange(N)/100; ridge
    normal equations solved by least squares (rl/maml_trpo.py:85 passes env.action_size as ``reg``)."""

    def __init__(self, input_size, reg=1e-5):
        self.input_size, self.reg = input_size, reg
        self._weight, self._weight_dev = np.zeros((2 * input_size + 4, 1)), None

    @property
    def weight(self):
        """The last fitted weights.  A fit done on the GPU (mi_gae_advantages) leaves them on the device; they are fetched on demand."""
        if self._weight_dev is not None:
            self._weight, self._weight_dev = self._weight_dev.detach().cpu().numpy().astype(np.float64).reshape(-1, 1), None
        return self._weight

    @weight.setter
    def weight(self, value):
        self._weight, self._weight_dev = value, None

    def _features(self, states):
        n = states.shape[0]
        al = (np.arange(n, dtype=np.float64) / 100.0).reshape(-1, 1)
        return np.concatenate([states, states ** 2, al, al ** 2, al ** 3, np.ones((n, 1))], axis=1)

    def fit(self, states, returns):
        f = self._features(_np(states))
        a = f.T @ f + self.reg * np.eye(f.shape[1])
        self.weight = np.linalg.lstsq(a, f.T @ _np(returns), rcond=None)[0]

    def __call__(self, states):
        return self._features(_np(states)) @ self.weight


def compute_advantages(baseline, tau, gamma, rewards, dones, states, next_states, update_vf=True):
    """reference rl.py:95-110 (GAE with cherry semantics).  numpy float64 [N,1]."""
    rewards, dones = _np(rewards), _np(dones)
    returns = discount(gamma, rewards, dones)
    if update_vf:
        baseline.fit(states, returns)
    values, next_values = baseline(states), baseline(next_states)
    bootstraps = values * (1.0 - dones) + next_values * dones
    nxt = np.concatenate([bootstraps[1:], np.zeros((1, 1))], axis=0)
    td = rewards + gamma * (1.0 - dones) * nxt - bootstraps
    return discount(gamma * tau, td, dones)


def normalize(x, epsilon=1e-8):
    """cherry.normalize"""
    return (x - x.mean()) / (x.std(ddof=1) + epsilon) if x.size > 1 else x


_ch_normalize = normalize                                      # (``_batch_advantages`` has a switch of that name)


def _host_replays(replay_list):
    """Replays (dicts of device tensors) -> dicts of float64 numpy arrays with ONE device-to-host copy per field for the whole list
    (a copy per replay and field costs a stream synchronisation each: 240 of them for 20 tasks x 2 replays)."""
    keys = ('states', 'actions', 'rewards', 'dones', 'next_states')
    lens = [int(r['states'].shape[0]) for r in replay_list]
    out = [dict() for _ in replay_list]
    for k in keys:
        parts = [r[k].detach().reshape(r[k].shape[0], -1) if torch.is_tensor(r[k]) else torch.as_tensor(np.asarray(r[k])).reshape(len(r[k]), -1)
                 for r in replay_list]
        big = torch.cat([q.to(parts[0].device, torch.float64) for q in parts]).cpu().numpy()
        off = 0
        for o, n in zip(out, lens):
            o[k] = big[off:off + n]
            off += n
    return out


def _device_batch(replay_list, S, A, dev):
    """Replays (dicts of tensors / arrays) -> one padded fp32 device batch {states [R,B,S], actions [R,B,A], next_states, rewards
    [R,B], dones [R,B], count [R] int32}, assembled ON the device: one stack per field, no host round trip."""
    lens = [int(r['states'].shape[0]) for r in replay_list]
    B = max(lens)

    # fast path: every field of every replay already a contiguous fp32 tensor on the device -- mi_copy_segments packs all five fields of all
    # replays (padding rows zeroed) in one launch per 128 arrays, the host collects 5 R addresses (the concatenate / pad / gather per field
    # of the general path below is 0.5 ms of host time for the 40 ragged replays of a 20-task meta-iteration)
    packed = _device_batch_packed(replay_list, lens, B, S, A, dev)
    if packed is not None:
        return packed

    ragged = any(n != B for n in lens)
    if ragged:          # one row index for all fields: replay r's rows, then the appended zero row for its padding
        total = sum(lens)
        idx = np.full((len(lens), B), total, dtype=np.int64)
        off = 0
        for i, n in enumerate(lens):
            idx[i, :n] = np.arange(off, off + n)
            off += n
        idx = torch.from_numpy(idx.reshape(-1)).to(dev)
    first = replay_list[0]['states']
    plain = (not ragged and torch.is_tensor(first) and first.device == torch.device(dev) and
             all(torch.is_tensor(r[k]) and r[k].dtype == torch.float32 and r[k].device == first.device and r[k].is_contiguous()
                 for r in replay_list for k in ('states', 'actions', 'next_states', 'rewards', 'dones')))
    if plain:
        R = len(lens)
        out = {k: torch.stack([r[k].detach() for r in replay_list]).reshape(R, B, w)
               for k, w in (('states', S), ('actions', A), ('next_states', S))}
        out['rewards'] = torch.stack([r['rewards'].detach() for r in replay_list]).reshape(R, B)
        out['dones'] = torch.stack([r['dones'].detach() for r in replay_list]).reshape(R, B)
        out['count'] = torch.full((R,), B, dtype=torch.int32, device=dev)
        return out

    def field(k, width):
        parts = []
        for r, n in zip(replay_list, lens):
            t = r[k] if torch.is_tensor(r[k]) else torch.as_tensor(np.asarray(r[k]))
            parts.append(t.detach().to(dev, torch.float32).reshape(n, width))
        if not ragged:
            return torch.stack(parts).contiguous()
        # ragged replays (episodes that end early): concatenate, append a zero row, gather -- 3 launches per field instead of one
        # pad per replay
        flat = torch.nn.functional.pad(torch.cat(parts), (0, 0, 0, 1))
        return flat.index_select(0, idx).view(len(lens), B, width)

    out = dict(states=field('states', S), actions=field('actions', A), next_states=field('next_states', S),
               rewards=field('rewards', 1).reshape(len(lens), B), dones=field('dones', 1).reshape(len(lens), B))
    out['count'] = torch.tensor(lens, dtype=torch.int32, device=dev)
    return out


_FIELDS = ('states', 'actions', 'next_states', 'rewards', 'dones')


class Replay(dict):
    """A replay as the runners of this package return it: a dict of tensors that remembers the device addresses of its five fields once
    ``_device_batch_packed`` has checked them (fp32, contiguous, on the device), so the meta-step that gathers the same replays again
    reads one tuple per replay instead of inspecting five tensors.  Any change of the dict's entries forgets it; plain dicts work as before."""
    __slots__ = ('_mi_pack',)

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._mi_pack = None

    def _forget(self):
        self._mi_pack = None

    def __setitem__(self, k, v):
        self._mi_pack = None
        super().__setitem__(k, v)

    def __delitem__(self, k):
        self._mi_pack = None
        super().__delitem__(k)

    def update(self, *a, **k):
        self._mi_pack = None
        super().update(*a, **k)

    def pop(self, *a):
        self._mi_pack = None
        return super().pop(*a)

    def popitem(self):
        self._mi_pack = None
        return super().popitem()

    def clear(self):
        self._mi_pack = None
        super().clear()

    def setdefault(self, *a):
        self._mi_pack = None
        return super().setdefault(*a)

    def __ior__(self, other):
        self._mi_pack = None
        return super().__ior__(other)

    def __reduce_ex__(self, protocol):
        # pickling (torch.save, multiprocessing) must not carry the remembered device ADDRESSES: the restored tensors live elsewhere
        return (Replay, (dict(self),))


def _device_batch_packed(replay_list, lens, B, S, A, dev):
    """_device_batch through mi_copy_segments, or None when a field is not a contiguous fp32 tensor on ``dev`` (the general path converts)."""
    dev = torch.device(dev)
    if dev.type != 'cuda':
        return None
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    R = len(lens)
    widths = (S, A, S, 1, 1)
    f32, Tensor, didx = torch.float32, torch.Tensor, dev.index
    srcs, cnts = [], []
    key = (didx, S, A)
    for r, n in zip(replay_list, lens):           # (attribute reads only: this loop is the host time of the call, ~0.8 us per array)
        memo = r._mi_pack if type(r) is Replay else None
        if memo is not None and memo[0] == key and memo[1] == n:
            srcs.extend(memo[2])                  # (checked before; the tensors are held by the replay, so the addresses are theirs)
            cnts.extend(memo[3])
            continue
        ps, cs = [], []
        for k, w in zip(_FIELDS, widths):
            t = r[k]
            if not (isinstance(t, Tensor) and t.dtype is f32 and t.is_cuda and t.get_device() == didx and t.is_contiguous() and t.numel() == n * w):
                return None
            ps.append(t.data_ptr())
            cs.append(n * w)
        if type(r) is Replay:
            r._mi_pack = (key, n, tuple(ps), tuple(cs))
        srcs.extend(ps)
        cnts.extend(cs)
    out = dict(states=torch.empty(R, B, S, dtype=f32, device=dev), actions=torch.empty(R, B, A, dtype=f32, device=dev),
               next_states=torch.empty(R, B, S, dtype=f32, device=dev), rewards=torch.empty(R, B, dtype=f32, device=dev),
               dones=torch.empty(R, B, dtype=f32, device=dev))
    base = [out[k].data_ptr() for k in _FIELDS]
    dsts, pads = [], []
    for i in range(R):
        for b, w in zip(base, widths):
            dsts.append(b + 4 * i * B * w)
            pads.append(B * w)
    from ..engine import copy_segments, upload_int32
    copy_segments(srcs, dsts, cnts, pads, dev)
    if all(n == B for n in lens):
        out['count'] = torch.full((R,), B, dtype=torch.int32, device=dev)
    else:
        out['count'] = upload_int32(lens, dev)
    return out


def _stacked_flat_parameters(policies, dev):
    """[len(policies), P] fp32: every policy's parameters in the engine's order (sigma first), gathered by mi_copy_segments from the
    parameter tensors where they lie; None when one of them is not a contiguous fp32 tensor on ``dev``."""
    dev = torch.device(dev)
    if dev.type != 'cuda':
        return None
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    f32, didx = torch.float32, dev.index
    srcs, cnts, offs, P = [], [], [], None
    for row, p in enumerate(policies):
        off = 0
        for q in p._engine_params():
            if not (q.dtype is f32 and q.is_cuda and q.get_device() == didx and q.is_contiguous()):
                return None
            n = q.numel()
            srcs.append(q.data_ptr())
            cnts.append(n)
            offs.append((row, off))                        # (the row travels with the segment: policies may split P differently)
            off += n
        if P is None:
            P = off
        elif off != P:
            return None
    out = torch.empty(len(policies), P, dtype=f32, device=dev)
    base = out.data_ptr()
    dsts = [base + 4 * (row * P + o) for row, o in offs]
    from ..engine import copy_segments
    copy_segments(srcs, dsts, cnts, cnts, dev)
    return out


def _replay_batch(replay_list, S, A, dev):
    """``_device_batch`` that remembers the replays it came from (key 'replays'): the host walk of ``_batch_advantages`` reads their
    own arrays, not the fp32 batch."""
    batch = _device_batch(replay_list, S, A, dev)
    batch['replays'] = replay_list
    return batch


def _stack_batches(sups, qry):
    """Padded support batches and the query batch, each with its advantages under 'adv' -> (sup, qry) as the engine takes them:
    sup {states [N,R,B,S], actions [N,R,B,A], adv [N,R,B], done [N,R,B], count [N,R]} (None without support batches), qry the
    same without the N axis, at their common padded length B -- a shorter batch gets zero rows appended.  Batches of device
    rollouts have one length: nothing is padded there and the query's tensors are returned as they lie."""
    B = max(b['states'].shape[1] for b in sups + [qry])

    def fit(b):
        n = B - b['states'].shape[1]
        pad = lambda t: t if n == 0 else torch.nn.functional.pad(t, [0, 0] * (t.dim() - 2) + [0, n])
        return dict(states=pad(b['states']), actions=pad(b['actions']), adv=pad(b['adv']), done=pad(b['dones']), count=b['count'])

    sups, qry = [fit(b) for b in sups], fit(qry)
    return ({k: torch.stack([b[k] for b in sups]) for k in qry} if sups else None), qry


def _gae_max_rows(S):
    from ..engine import gae_max_rows
    return gae_max_rows(S)


def _gae_on_device(dev, S, rows):
    return torch.device(dev).type == 'cuda' and 0 < rows <= _gae_max_rows(S)


def _batch_advantages(batch, baseline, gamma, tau, normalize=True, fit=True, weights=None):
    """compute_advantages (+ ch.normalize) (rl.py:95-110,355) of every replay of a padded batch -> (adv [R, B] fp32 on the batch's
    device, the fitted baseline weights [R, 2S+4] fp64 or None).  THE place that chooses between mi_gae_advantages (one launch for
    all replays) and the host numpy walk (replays the kernel cannot hold, no GPU).  ``fit``: re-fit the baseline per replay, which
    leaves it fitted to the LAST one as after the reference's replay-by-replay walk; False evaluates with ``weights`` [R, 2S+4]
    (each replay its own) or, without them, with the baseline as last fitted (update_vf=False, rl.py:401).  The host walk reads the
    replays the batch came from (``_replay_batch``; the rows of the batch itself where it carries none) in fp64."""
    R, B, S = batch['states'].shape
    dev = batch['states'].device
    if _gae_on_device(dev, S, B):
        from ..engine import gae_advantages
        if not fit and weights is None:
            weights = baseline._weight_dev if baseline._weight_dev is not None else torch.from_numpy(np.ascontiguousarray(baseline.weight))
            weights = weights.reshape(1, -1).expand(R, -1)
        adv, wts = gae_advantages(batch['states'], batch['next_states'], batch['rewards'], batch['dones'], batch['count'], gamma, tau,
                                  baseline.reg, normalize=normalize, want_weights=True, weights=None if fit else weights)
        if fit:
            baseline._weight_dev = wts[-1]
        return adv, wts
    if weights is not None:
        raise ValueError('per-replay baseline weights are taken by mi_gae_advantages only')
    replays = batch.get('replays') or [_replay_rows(batch, i, n) for i, n in enumerate(batch['count'].tolist())]
    adv = np.zeros((R, B), np.float32)
    for i, ep in enumerate(_host_replays(replays)):
        a = compute_advantages(baseline, tau, gamma, ep['rewards'], ep['dones'], ep['states'], ep['next_states'], fit)
        adv[i, :a.shape[0]] = (_ch_normalize(a) if normalize else a).reshape(-1)
    return torch.from_numpy(adv).to(dev), None


# ---------------------------------------------------------------------------------------------- reference functions
def trpo_a2c_loss(episodes, learner, baseline, gamma, tau, update_vf=True):
    """reference rl.py:346-358: -mean(log_prob * normalised advantages).  A value with the bare policy (the gradient path is trpo_update);
    ``learner.log_prob`` of a ``MAML`` wrapper carries a graph while grad mode is on (core_functions/maml.py), and so does this loss."""
    b = _replay_batch([_as_replay(episodes)], learner.input_size, learner.output_size, learner.sigma.device)
    adv, _ = _batch_advantages(b, baseline, gamma, tau, fit=update_vf)
    lp = learner.log_prob(b['states'][0], b['actions'][0])
    return -(lp * adv[0].reshape(-1, 1).to(lp)).mean()


def _trpo_step(eng, inner_lr, head_only, table=None, step_row=None):
    """``step`` of the adapt loop for TRPO: mi_policy_adapt, or with a step-size ``table`` [rows, P] (``_trpo_lr_table``)
    mi_policy_adapt_lr with the row ``step_row[k]`` of adapt step k."""
    return lambda theta, b, adv, k=0: eng.adapt(theta, b['states'], b['actions'], adv, b['count'],
                                                inner_lr if table is None else table[step_row[k]], head_only=head_only)[0]


def _trpo_lr_table(learner, name):
    """The FIXED step-size table [rows, P] (fp32, engine order, on the policy's device) of a ``MAML`` wrapper that holds more than one
    number -- a non-learnable ``InnerLR``, or a number with ``allow_nograd`` around a policy with frozen parameters; None for the bare
    policy or a wrapper with one number (``params['inner_lr']`` is the step).  Steps that require grad are refused: TRPO's outer step is
    a trust region over theta alone, and their gradient would have to enter the KL's curvature product as well."""
    lrv = _policy_lr_vector(learner)
    if lrv is None:
        return None
    if lrv.requires_grad:
        raise ValueError(f"{name}: per-parameter inner-loop step sizes (an InnerLR, or allow_nograd) are taken by the VPG / PPO / DiCE "
                         "calls only; the TRPO calls adapt with the one number params['inner_lr'] -- wrap the policy as MAML(policy, lr=number)"
                         " -- or with FIXED steps: an InnerLR(learnable=False) is accepted, a learnable one is not")
    return lrv.detach().to(_unwrap(learner).sigma.device, torch.float32).contiguous()


def trpo_update(episodes, learner, baseline, inner_lr, gamma, tau, anil=False, first_order=False):
    """reference rl.py:361-374: one MAML update of the policy on ``episodes``; returns the adapted policy (a new object; the
    second-order dependence on the original parameters is handled inside meta_optimize_trpo's fused calls)."""
    # anil only sets allow_unused (rl.py:371): which parameters move is decided by the policy's own switch -- with
    # DiagNormalPolicyANIL.turn_off_body_grads() the body's gradients are None and maml_update leaves it unchanged.
    table = _trpo_lr_table(learner, 'trpo_update')
    b = _replay_batch([_as_replay(episodes)], learner.input_size, learner.output_size, learner.sigma.device)
    adv, _ = _batch_advantages(b, baseline, gamma, tau)
    row = 0
    if table is not None and table.shape[0] > 1:              # the row the step-wise learner's ``adapt`` would read
        row = int(getattr(learner, '_steps_done', 0))
        if row >= table.shape[0]:
            raise ValueError(f'trpo_update: this learner holds step sizes for {table.shape[0]} inner steps and has taken {row}')
    step = _trpo_step(learner.engine(), inner_lr, bool(getattr(learner, 'features_no_grad', False)), table, [row])
    new = deepcopy(learner)
    new.load_flat(step(learner.flat(), b, adv)[0])
    if table is not None:
        new.__dict__['_steps_done'] = row + 1
    return new


def _adapt_loop(run, step, theta, steps, baseline, gamma, tau, normalize, keep_views=False):
    """THE adapt loop of fast_adapt_trpo / _vpg / _ppo and their ``*_tasks`` forms: ``steps`` support steps -- ``run(k, theta)`` rolls
    out a padded batch with the parameters so far ([P] shared, or [R, P]), its advantages are taken with the baseline re-fitted
    (``_batch_advantages``, ``normalize`` as given), ``step(theta, batch, adv, k)`` returns the updated parameters [R, P] -- and the
    query run.  Returns (theta after the last step, the support batches with their advantages under 'adv', the query batch, the
    baseline weights [R, 2S+4] of the last fit or None, and with ``keep_views`` per replay row the ``Replay`` views of its runs --
    one read of the row counts per run, the only synchronisation of the loop -- else None)."""
    sups, wts, views = [], None, None
    for k in range(steps + 1):
        batch = run(k, theta)
        if keep_views:
            counts = batch['count'].tolist()
            views = views or [[] for _ in counts]
            for i, n in enumerate(counts):
                views[i].append(_replay_rows(batch, i, n))
        if k == steps:
            return theta, sups, batch, wts, views
        batch['adv'], wts = _batch_advantages(batch, baseline, gamma, tau, normalize=normalize)
        sups.append(batch)
        theta = step(theta, batch, batch['adv'], k)


class _TaskWalk:
    """``run`` of the adapt loop for ONE task and any runner with ``run(policy, episodes)``: run 0 acts with ``actor`` itself, run k
    with a copy of the previous actor that holds theta_k.  ``before_query(actor)`` is called ahead of the last run (ANIL switches
    the body gradients back on there, rl.py:395-396).  Keeps what the runner returned (``replays``) and the last actor (``current``)."""

    def __init__(self, task, actor, params, before_query=None):
        self.task, self.current, self.before_query = task, actor, before_query
        self.steps, self.episodes, self.replays = params['adapt_steps'], params['adapt_batch_size'], []

    def __call__(self, k, theta):
        if k:
            self.current = deepcopy(self.current)
            self.current.load_flat(theta[0])
        if k == self.steps and self.before_query is not None:
            self.before_query(self.current)
        self.replays.append(self.task.run(self.current, episodes=self.episodes))
        pol = _unwrap(self.current)
        return _replay_batch([_as_replay(self.replays[-1])], pol.input_size, pol.output_size, pol.sigma.device)


def fast_adapt_trpo(task, learner, baseline, params, anil=False, first_order=False, render=False):
    """reference rl.py:377-406.  ``task.run(policy, episodes=n)`` returns a replay (dict or cherry-style object, ``_as_replay``).
    ``learner``: the policy itself or a ``MAML`` wrapper around it (rl/anil_trpo.py:84 wraps; rl.py:382,396 reach the policy as
    ``learner.module``)."""
    table = _trpo_lr_table(learner, 'fast_adapt_trpo')
    step_row = None if table is None else _lr_step_rows(table.shape[0], params['adapt_steps'])
    if anil:                                                   # rl.py:381-382
        _unwrap(learner).turn_off_body_grads()
    walk = _TaskWalk(task, learner, params, (lambda actor: _unwrap(actor).turn_on_body_grads()) if anil else None)
    step = _trpo_step(learner.engine(), params['inner_lr'], bool(getattr(learner, 'features_no_grad', False)), table, step_row)
    _adapt_loop(walk, step, learner.flat(), params['adapt_steps'], baseline, params['gamma'], params['tau'], True)
    learner, task_replay = walk.current, walk.replays
    valid_loss = trpo_a2c_loss(task_replay[-1], learner, baseline, params['gamma'], params['tau'], update_vf=False)
    query_rew = _as_replay(task_replay[-1])['rewards'].sum().item() / params['adapt_batch_size']                    # rl.py:403
    query_success_rate = get_ep_successes(task_replay[-1], params.get('max_path_length')) / params['adapt_batch_size']  # rl.py:404
    return learner, valid_loss, task_replay, query_rew, query_success_rate


def _replay_rows(out, i, n):
    """Task i of a padded device batch (PolicyEngine.rollout) as a ``Replay`` of its leading n rows: contiguous fp32 views, so
    ``_device_batch_packed`` takes them as they lie."""
    return Replay(states=out['states'][i, :n], actions=out['actions'][i, :n], rewards=out['rewards'][i, :n].unsqueeze(1),
                  dones=out['dones'][i, :n].unsqueeze(1), next_states=out['next_states'][i, :n])


def _rollout_theta(policies_or_theta, dev):
    """(engine, theta [P] or [T, P]) from one policy (shared parameters), a sequence of policies (one per task), or a pair
    (policy or PolicyEngine, theta tensor)."""
    pt = policies_or_theta
    if isinstance(pt, tuple) and len(pt) == 2 and torch.is_tensor(pt[1]):
        eng = pt[0].engine() if hasattr(pt[0], 'engine') else pt[0]
        return eng, pt[1].detach().to(dev, torch.float32)
    if isinstance(pt, (list, tuple)):
        pols = [_unwrap(q) for q in pt]
        theta = _stacked_flat_parameters(pols, dev)
        if theta is None:
            theta = torch.stack([q.flat() for q in pols]).to(dev)
        return pols[0].engine(), theta
    pol = _unwrap(pt)
    return pol.engine(), pol.flat()


def rollout_tasks(policies_or_theta, goals, ids, seed, episodes, max_path_length, dev=None):
    """``episodes`` Particles2D episodes for every task of a meta-batch through ONE mi_particles_rollout call and one read-back of the
    tasks' row counts; returns the list of the tasks' ``Replay``s.  ``policies_or_theta``: one policy (every task acts with it), a
    sequence of policies (one per task), or ``(policy or PolicyEngine, theta [P] | [tasks, P])``.  Task i's rollout is a pure
    function of its parameters, ``goals[i]`` and ``(seed, ids[i])``."""
    eng, theta = _rollout_theta(policies_or_theta, dev or device)
    out = eng.rollout(theta, goals, ids, seed, episodes, max_path_length)
    return [_replay_rows(out, i, n) for i, n in enumerate(out['count'].tolist())]


def _rollout_run(name, pol, goals, params, seed, first_id, stride=None):
    """``run`` of the adapt loop for ALL tasks on device rollouts -> (tasks, run): run k is ONE mi_particles_rollout call with the
    tasks' parameters so far, task i under rollout id ``_task_rollout_ids(...)[k][i]``.  The goals and the ids of all
    (adapt_steps + 1) x tasks runs travel once, in kernel arguments (no pageable copy, no synchronisation).  Replays longer than
    mi_gae_advantages takes are refused up front: ``name`` keeps them on the device."""
    from ..engine import upload_int32, _as_i32
    eng, dev = pol.engine(), pol.sigma.device
    goals = np.ascontiguousarray(np.asarray(goals, dtype=np.float32).reshape(-1, 2))
    T, K, E, L = goals.shape[0], params['adapt_steps'], params['adapt_batch_size'], params['max_path_length']
    if T < 1:
        raise ValueError(f'{name}: no goals')
    if not _gae_on_device(dev, pol.input_size, E * L):
        raise ValueError(f'{name} keeps replays of {E} x {L} rows on the device; mi_gae_advantages takes at most '
                         f'{_gae_max_rows(pol.input_size)} rows')
    goals_dev = upload_int32(goals.view(np.int32).reshape(-1).tolist(), dev).view(torch.float32).view(T, 2)
    halves = []
    for row in _task_rollout_ids(int(first_id), T, K, stride):
        for r in row:
            r &= 2 ** 64 - 1
            halves += [_as_i32(r & 0xffffffff), _as_i32(r >> 32)]
    ids = upload_int32(halves, dev).view(torch.int64).view(K + 1, T)
    return T, lambda k, theta: eng.rollout(theta, goals_dev, ids[k], seed, E, L)


def fast_adapt_trpo_tasks(goals, policy, baseline, params, seed, first_id, anil=False, first_order=False):
    """``fast_adapt_trpo`` (reference rl.py:377-406) for ALL tasks of a meta-batch at once on device rollouts: per adapt step one
    rollout call, one mi_gae_advantages launch and one mi_policy_adapt call over all tasks, then one query rollout with per-task
    parameters.  Returns the list of the tasks' ``(learner, valid_loss, task_replay, query_rew, query_success_rate)``.  Task i's
    run k (the support steps, then the query) uses rollout id ``first_id + i * (adapt_steps + 1) + k`` -- what task i gets from
    ``fast_adapt_trpo`` with ``Particles2DRunner(goal, L, rollout='device', seed=seed, first_id=first_id + i * (adapt_steps + 1))``.
    ``baseline`` is left as after that task-by-task walk: fitted to the last task's last support replay."""
    table = _trpo_lr_table(policy, 'fast_adapt_trpo_tasks')
    step_row = None if table is None else _lr_step_rows(table.shape[0], params['adapt_steps'])
    pol = _unwrap(policy)
    T, run = _rollout_run('fast_adapt_trpo_tasks', pol, goals, params, seed, first_id)
    eng, A, E = pol.engine(), pol.output_size, params['adapt_batch_size']
    gamma, tau = params['gamma'], params['tau']
    if anil:                                                   # rl.py:381-382: the inner loop moves the head only
        pol.turn_off_body_grads()
    head_only = bool(getattr(pol, 'features_no_grad', False))
    if anil:                                                   # rl.py:395-396
        pol.turn_on_body_grads()
    theta, _, out, wts, replays = _adapt_loop(run, _trpo_step(eng, params['inner_lr'], head_only, table, step_row), pol.flat(),
                                              params['adapt_steps'], baseline, gamma, tau, True, keep_views=True)
    # the query replay's loss with each task's own baseline, as fitted to its last support replay (update_vf=False, rl.py:401)
    adv, _ = _batch_advantages(out, baseline, gamma, tau, fit=False, weights=wts)
    thetas = theta if theta.dim() == 2 else theta.unsqueeze(0).expand(T, -1)
    loc = eng.forward(theta, out['states'])
    scale = torch.exp(torch.clamp(thetas[:, :A], min=float(np.log(1e-6))))
    query_rew = (out['rewards'].sum(dim=1) / E).tolist()
    results = []
    for i, task_replay in enumerate(replays):
        n = task_replay[-1]['states'].shape[0]
        learner = deepcopy(pol)
        learner.load_flat(thetas[i].contiguous())
        # trpo_a2c_loss's own expressions on the task's rows (rl.py:346-358)
        lp = torch.distributions.Normal(loc=loc[i, :n], scale=scale[i]).log_prob(out['actions'][i, :n]).mean(dim=1, keepdim=True)
        valid_loss = -(lp * adv[i, :n].reshape(-1, 1)).mean()
        suc = get_ep_successes(task_replay[-1], params.get('max_path_length')) / E
        results.append((learner, valid_loss, task_replay, query_rew[i], suc))
    return results


class _SurrogateContext:
    """Everything meta_surrogate_loss needs that does not depend on the candidate parameters (advantages are functions of
    the replays only -- the reference re-fits the baseline to the same data on every call, rl.py:99,465)."""

    def __init__(self, iter_replays, iter_policies, policy, baseline, params):
        S, A, dev = policy.input_size, policy.output_size, policy.sigma.device
        iter_replays = [[_as_replay(r) for r in task] for task in iter_replays]
        K = len(iter_replays[0]) - 1
        if K < 1 or any(len(r) != K + 1 for r in iter_replays):
            raise ValueError('every task needs the same number (>= 1) of support replays plus one query replay')
        self.steps = K
        nT = len(iter_replays)
        flat = [r[k] for k in range(K + 1) for r in iter_replays]                    # [k][task]
        # advantages of all (K + 1) x tasks replays in ONE launch, the batch assembled on the device (the reference re-fits the
        # baseline and re-runs GAE per task and replay on the CPU at every evaluation of the surrogate, rl.py:444-465); the order
        # of the replays is immaterial to them, the baseline being re-fitted per replay
        batch = _replay_batch(flat, S, A, dev)
        advs, _ = _batch_advantages(batch, baseline, params['gamma'], params['tau'])
        rows = dict(states=batch['states'], actions=batch['actions'], adv=advs, count=batch['count'], done=batch['dones'])
        self.qry = {k: v[K * nT:] for k, v in rows.items()}
        # the K support replays are the batch's first K x tasks rows: [K, T, ...] views, no copy (leading rows: contiguous as they lie)
        self.sup = {k: v[:K * nT].unflatten(0, (K, nT)) for k, v in rows.items() if k != 'done'}
        self.engine = policy.engine()
        # the stored old policies' parameters as ONE gather ([tasks, P], engine order: sigma first) and their scales from its first columns
        # (per-policy flat() / clamp / exp launches were ~80 of the ~100 launches of this constructor)
        if all(hasattr(p, '_engine_params') for p in iter_policies):
            thetas = _stacked_flat_parameters(iter_policies, dev)
            if thetas is None:
                thetas = torch.cat([q.detach().reshape(-1).float() for p in iter_policies for q in p._engine_params()]).view(len(iter_policies), -1)
        else:                                                       # any object with the policy protocol (flat(), sigma first)
            thetas = torch.stack([p.flat() for p in iter_policies])
        self.old_loc = self.engine.forward(thetas, self.qry['states'])
        self.old_scale = torch.exp(torch.clamp(thetas[:, :A], min=float(np.log(1e-6)))).contiguous()
        # the step of every engine call: the number, or the fixed step-size table of a MAML wrapper (``_trpo_lr_table``) with the row
        # each update reads.  The surrogate re-adapts with the table as it is (the reference replays the inner step with every
        # parameter, rl.py:447-453), whatever head mask the stored old policies were adapted with.
        table = _trpo_lr_table(policy, 'meta_surrogate_loss')
        self.inner_lr = params['inner_lr'] if table is None else table
        self.lr_rows = {} if table is None else {'step_lr_row': _lr_step_rows(table.shape[0], K)}     # (only the table's calls name the rows)

    # Multi-GPU (TRPO): every rank holds a shard of the task list; the mean over tasks of (loss, kl, grad) and
    # of each Fisher-vector product is completed by one small all-reduce per evaluation (RCCL; 42 KB for the 2x100 policy).
    def _allmean(self, *tensors):
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return tensors
        n_local = float(self.qry['states'].shape[0])
        flat = torch.cat([t.reshape(-1) for t in tensors] + [torch.ones(1, device=tensors[0].device)]) * n_local
        dist.all_reduce(flat)
        flat = flat / flat[-1]
        out, off = [], 0
        for t in tensors:
            out.append(flat[off:off + t.numel()].view_as(t))
            off += t.numel()
        return tuple(out)

    def evaluate(self, theta, want_grad=False):
        loss, kl, grad = self.engine.surrogate(theta, self.sup, self.qry, self.old_loc, self.old_scale, self.inner_lr, want_grad,
                                               **self.lr_rows)
        if grad is None:
            loss, kl = self._allmean(loss, kl)
        else:
            loss, kl, grad = self._allmean(loss, kl, grad)
        return loss, kl, grad

    def prepare_general_kl(self, theta, want_grad=False):
        """ANIL-TRPO: the re-adapted policies differ from the stored old ones, the Fisher form does not apply; set up the exact
        KL Hessian-vector product (``PolicyEngine.kl_prepare``) at the theta of the preceding ``evaluate``.  ``theta`` is not
        read: the engine kept it.  Returns d mean KL / d theta if ``want_grad``."""
        grad = self.engine.kl_prepare(self.sup, self.qry, self.old_loc, self.old_scale, self.inner_lr, want_grad, **self.lr_rows)
        self.general = True
        return None if grad is None else self._allmean(grad)[0]

    def fvp(self, theta, v, damping=1e-5):
        """The curvature product at the theta of the preceding ``evaluate`` (``theta`` is not read: the engine kept it)."""
        # the damping term is linear in v, so averaging the per-rank results keeps it exact
        if getattr(self, 'general', False):
            return self._allmean(self.engine.fvp_general(self.sup, self.qry, self.old_scale, self.inner_lr, damping, v, **self.lr_rows))[0]
        return self._allmean(self.engine.fvp(self.sup, self.qry, self.inner_lr, damping, v, **self.lr_rows))[0]


def meta_surrogate_loss(iter_replays, iter_policies, policy, baseline, params, anil=False):
    """reference rl.py:441-473 -> (mean surrogate loss, mean KL) as 0-dim tensors."""
    ctx = _SurrogateContext(iter_replays, iter_policies, policy, baseline, params)
    loss, kl, _ = ctx.evaluate(policy.flat())
    return loss[0], kl[0]


def conjugate_gradient(Ax, b, num_iterations=10, tol=1e-10, eps=1e-8):
    """cherry.algorithms.trpo.conjugate_gradient (reference rl.py:418).  The recurrences (dot products, axpys on 10,604
    elements) are carried in fp64 on the device; every A p is one fp32 Fisher-vector product through the engine."""
    dt = b.dtype
    if b.is_cuda:
        return _conjugate_gradient_device(Ax, b, num_iterations, tol, eps)
    b = b.double()
    x = torch.zeros_like(b)
    r, p = b.clone(), b.clone()
    r_dot_old = torch.dot(r, r)
    for _ in range(num_iterations):
        Ap = Ax(p.to(dt)).double()
        alpha = r_dot_old / (torch.dot(p, Ap) + eps)
        x += alpha * p
        r -= alpha * Ap
        r_dot_new = torch.dot(r, r)
        p = r + (r_dot_new / r_dot_old) * p
        r_dot_old = r_dot_new
        if r_dot_new.item() < tol:
            break
    return x.to(dt)


def _conjugate_gradient_device(Ax, b, num_iterations, tol, eps):
    """The same recurrences with the whole loop body after `Ap = Ax(p)` as one launch (mi_cg_update_checked)."""
    from .. import _lib
    from ..engine import _ptr, _stream
    lib = _lib.load()
    dev, n = b.device, b.numel()
    if b.dtype == torch.float32:
        b32 = b.detach().reshape(-1).contiguous()
        x, r, p = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        p32 = torch.empty(n, dtype=torch.float32, device=dev)
        rr = torch.empty(3, dtype=torch.float64, device=dev)      # r.r, last step length, "converged" latch
        with torch.cuda.device(dev):                              # x = 0, r = p = b, rr = (b.b, 0, 0): one launch
            _lib.check(lib.mi_cg_init(_stream(dev), _ptr(b32), _ptr(x), _ptr(r), _ptr(p), _ptr(p32), _ptr(rr), n))
    else:
        r = b.detach().to(torch.float64, copy=True).reshape(-1).contiguous()      # a copy: mi_cg_update overwrites r in place
        x, p = torch.zeros_like(r), r.clone()
        p32 = r.float()
        rr = torch.zeros(3, dtype=torch.float64, device=dev)
        rr[0] = torch.dot(r, r)
    for _ in range(num_iterations):
        # the reference's `if r_dot_new < tol: break` is taken on the device (mi_cg_update_checked): after the break every later
        # recurrence is a no-op, so the loop needs no host synchronisation per iteration and x is exactly the x at the break
        ap = Ax(p32.to(b.dtype)).detach().float().reshape(-1).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.mi_cg_update_checked(_stream(dev), _ptr(x), _ptr(r), _ptr(p), _ptr(ap), _ptr(rr), _ptr(p32), n, float(eps), float(tol)))
    return x.to(b.dtype).reshape(b.shape)


def meta_optimize_trpo(params, policy, baseline, iter_replays, iter_policies, anil=False):
    """reference rl.py:409-438: CG step direction from the Fisher-vector product of the mean KL, then backtracking line
    search on (surrogate loss, KL); updates ``policy`` in place.  Returns diagnostics."""
    _trpo_lr_table(policy, 'meta_optimize_trpo')            # (a learnable wrapper is refused under this function's name)
    ctx = _SurrogateContext(iter_replays, iter_policies, policy, baseline, params)
    theta = policy.flat()
    old_loss, old_kl, grad = ctx.evaluate(theta, want_grad=True)
    if anil:
        # The reference's surrogate replays the inner step with ALL parameters (clone_module(policy) has its body grads on,
        # rl.py:447-453) while the stored old policies were adapted head-only (rl.py:381-382): at the current parameters the new
        # policies differ from the old ones, KL's gradient is not zero, and trpo.hessian_vector_product(kl) is the exact Hessian
        # of the mean KL including the third derivative of the inner loss (``PolicyEngine.fvp_general``).
        ctx.prepare_general_kl(theta)
    Fvp = lambda v: ctx.fvp(theta, v)
    step = conjugate_gradient(Fvp, grad)
    if step.is_cuda and step.dtype == torch.float32:
        # shs = 0.5 step . F step, lagrange = sqrt(shs / max_kl), step / lagrange (rl.py:419-421) as one launch
        from .. import _lib
        from ..engine import _ptr, _stream
        step, fstep = step.contiguous(), Fvp(step).detach().float().reshape(-1).contiguous()
        scaled = torch.empty_like(step)
        with torch.cuda.device(step.device):
            _lib.check(_lib.load().mi_trpo_scale_step(_stream(step.device), _ptr(step), _ptr(fstep), step.numel(), float(params['max_kl']),
                                                      _ptr(scaled), None))
        step = scaled
    else:
        shs = 0.5 * torch.dot(step, Fvp(step))
        lagrange_multiplier = torch.sqrt(shs / params['max_kl'])
        step = step / lagrange_multiplier
    accepted, new_loss, kl = None, None, None
    for ls_step in range(params['ls_max_steps']):
        stepsize = params['backtrack_factor'] ** ls_step * params['outer_lr']
        cand = torch.add(theta, step, alpha=-stepsize).contiguous()
        new_loss, kl, _ = ctx.evaluate(cand)
        # (one host read for the three scalars of the test: each .item() is a copy and a synchronisation of its own, ~25 us)
        nl, ol, klv = torch.cat([new_loss.reshape(-1)[:1], old_loss.reshape(-1)[:1], kl.reshape(-1)[:1]]).tolist()
        if nl < ol and klv < params['max_kl']:
            policy.load_flat(cand)
            accepted = ls_step
            break
    return dict(grad=grad, step=step, old_loss=old_loss[0], old_kl=old_kl[0], accepted=accepted,
                new_loss=None if new_loss is None else new_loss[0], kl=None if kl is None else kl[0], fvp=Fvp, context=ctx)


# ---------------------------------------------------------------------------------------------- VPG / PPO (reference rl.py:209-337)
def _unwrap(learner):
    return getattr(learner, 'module', learner)


class _PolicyMetaLoss(torch.autograd.Function):
    """Validation loss of one task whose gradient w.r.t. the policy parameters came out of the same fused call
    (mi_policy_meta_batch); `.backward()` accumulates it like the reference's autograd graph through learner.adapt."""

    @staticmethod
    def forward(ctx, loss, grad, shapes, *params):
        ctx.shapes = shapes
        ctx.save_for_backward(grad)
        return loss.clone()

    @staticmethod
    def backward(ctx, gout):
        (grad,) = ctx.saved_tensors
        outs, off = [], 0
        for shp in ctx.shapes:
            n = int(torch.Size(shp).numel())
            outs.append((grad[off:off + n] * gout).reshape(shp))
            off += n
        return (None, None, None) + tuple(outs)


def _policy_lr_vector(learner):
    """The step sizes [rows, P] (engine order, connected to a learnable ``InnerLR``) of a ``MAML`` wrapper that holds more than one
    number for its policy; None for everything else -- the bare policy, a wrapper with a number: ``params['inner_lr']`` is the step."""
    if not (hasattr(learner, 'lr_flat') and hasattr(learner, 'module')):
        return None
    if learner.offsets_flat() is not None:
        raise NotImplementedError('per-step offsets are implemented for the fused MAML vision call, not for the policy calls')
    return learner.lr_flat()


def _lr_step_rows(lr_rows, adapt_steps):
    """The row of the step-size table each adapt step reads: its own with one row per adapt step, row 0 with one row for all."""
    if lr_rows not in (1, adapt_steps):
        raise ValueError(f'the learner holds step sizes for {lr_rows} inner steps; adapt_steps is {adapt_steps} '
                         '(InnerLR(steps=...) must be 1 or adapt_steps)')
    return [s if lr_rows > 1 else 0 for s in range(adapt_steps)]


def _refuse_lr_vector(learner, name):
    """TRPO's outer step is a trust region over theta alone and its fused calls take one number: no silent fall-back to it."""
    if _policy_lr_vector(learner) is not None:
        raise ValueError(f"{name}: per-parameter inner-loop step sizes (an InnerLR, or allow_nograd) are taken by the VPG / PPO / DiCE "
                         "calls only; the TRPO calls adapt with the one number params['inner_lr'] -- wrap the policy as MAML(policy, lr=number)")


def _adapt_and_validate(run, pol, baseline, params, algo, anil, first_order, dice, keep_views=False, learner=None):
    """fast_adapt_vpg / fast_adapt_ppo (reference rl.py:231-255,267-318) for the R replay rows ``run`` rolls out -- all tasks of a
    meta-batch (``_rollout_run``) or one (``_TaskWalk``): the adapt loop with one mi_policy_update call per step (``ppo_epochs``
    epochs for PPO), the query's advantages (fitted like the others; normalised for PPO only, vpg_a2c_loss does not, rl.py:217),
    then ONE mi_policy_meta_batch call from the shared parameters over the support batches and the query.  Returns (the summed
    validation loss, 0-dim, whose ``.backward()`` accumulates the summed meta-gradient; the losses [R]; the adapted parameters the
    query was rolled out with, [R, P] or the shared [P] without adapt steps; the query batch; the ``Replay`` views or None).
    ``learner``: what the caller was handed.  A ``MAML`` wrapper with per-parameter step sizes (``_policy_lr_vector``) takes the vector
    calls (mi_policy_update_lr / mi_policy_meta_batch_lr): adapt step s reads row s of an ``InnerLR`` with ``steps == adapt_steps``,
    row 0 of one with ``steps == 1`` (PPO's epochs share their adapt step's row), and ``.backward()`` also fills ``InnerLR.values.grad``."""
    eng = pol.engine()
    gamma, tau, lr = params['gamma'], params['tau'], params['inner_lr']
    epochs = params['ppo_epochs'] if algo == 'ppo' else 1
    clip = params.get('ppo_clip_ratio', 0.1)
    kind = 'ppo' if algo == 'ppo' else ('dice' if dice else 'a2c')
    lrv = _policy_lr_vector(learner)
    if lrv is not None:
        step_row = _lr_step_rows(lrv.shape[0], params['adapt_steps'])
        rows = lrv.detach().to(pol.sigma.device, torch.float32).contiguous()
    lr_of = lambda k: lr if lrv is None else rows[step_row[k]]          # the step of adapt step k: the number, or its row of the table
    step = lambda theta, b, adv, k: eng.update(theta, b['states'], b['actions'], adv, b['count'], lr_of(k), loss=kind, epochs=epochs, clip=clip,
                                               done=b['dones'] if kind == 'dice' else None, head_only=bool(anil))[0]
    theta0 = pol.flat()
    theta, sups, qry, _, views = _adapt_loop(run, step, theta0, params['adapt_steps'], baseline, gamma, tau, algo == 'ppo', keep_views)
    qry['adv'], _ = _batch_advantages(qry, baseline, gamma, tau, normalize=(algo == 'ppo'))
    sup, engine_qry = _stack_batches(sups, qry)
    step_batch = [b for b in range(len(sups)) for _ in range(epochs)]
    need = torch.is_grad_enabled() and any(q.requires_grad for q in pol.parameters())
    need_lr = lrv is not None and torch.is_grad_enabled() and lrv.requires_grad
    kw = dict(loss=kind, clip=clip, head_only=bool(anil), first_order=first_order, with_grad=need or need_lr)
    if lrv is None:
        (lt, _, grad), lr_grad = eng.meta_batch(theta0, sup, engine_qry, step_batch, lr, **kw), None
    else:
        lt, _, grad, lr_grad = eng.meta_batch_lr(theta0, sup, engine_qry, step_batch, rows, [step_row[b] for b in step_batch], want_lr_grad=need_lr, **kw)
    total = lt.sum()
    if need or need_lr:                                        # the step tensor is one more differentiable input: lr_grad * gout
        eparams = pol._engine_params() + ([lrv] if need_lr else [])
        flat = torch.cat([grad, lr_grad.reshape(-1)]) if need_lr else grad
        total = _PolicyMetaLoss.apply(total, flat, [q.shape for q in eparams], *eparams)
    return total, lt, theta, qry, views


def _adapt_task_walk(task, learner, baseline, params, algo, anil, first_order, dice=False):
    """``_adapt_and_validate`` for one task and any runner -> (valid_loss, query reward, success rate)."""
    pol = _unwrap(learner)
    if anil:
        pol.turn_off_body_grads()
    walk = _TaskWalk(task, pol, params, (lambda actor: pol.turn_on_body_grads()) if anil else None)
    valid_loss, _, _, _, _ = _adapt_and_validate(walk, pol, baseline, params, algo, anil, first_order, dice, learner=learner)
    query = _as_replay(walk.replays[-1])
    rew = query['rewards'].sum().item() / params['adapt_batch_size']
    suc = get_ep_successes(query, params.get('max_path_length')) / params['adapt_batch_size']                          # rl.py:252,315
    # learn2learn's learner.adapt updates the learner in place; here the base module is shared by every clone, so the adapted
    # parameters are handed over on the side (evaluate() below acts with them)
    try:
        learner._adapted_policy = walk.current
    except Exception:
        pass
    return valid_loss, rew, suc


def fast_adapt_vpg(task, learner, baseline, params, anil=False, first_order=False, render=False, dice=False):
    """reference rl.py:231-255 -> (valid_loss, query reward, success rate); `valid_loss.backward()` accumulates the MAML
    gradient (second order unless first_order) into the policy's parameters.  ``dice`` (not a parameter of the reference's
    fast_adapt_vpg, whose calls leave vpg_a2c_loss at dice=False): every vpg_a2c_loss of the adaptation -- the adapt losses and
    the validation loss -- uses the DiCE objective of rl.py:219-226."""
    return _adapt_task_walk(task, learner, baseline, params, 'vpg', anil, first_order, dice=dice)


def vpg_a2c_loss(episodes, learner, baseline, gamma, tau, dice=False):
    """reference rl.py:208-228: -mean(log_prob * advantages).  With a ``MAML`` wrapper as ``learner`` and grad mode on, the loss is
    differentiable in the learner's fast weights, to second order (``learner.adapt(vpg_a2c_loss(...))``, misc_scripts/cl_rl.py:71-75:
    mi_policy_vjp / mi_policy_hvp); with the bare policy it is a value (the fused gradient path is fast_adapt_vpg).
    ``dice``: -mean(magic_box(weighted_cumsum(log_probs, weights)) * advantages) = -mean(advantages) (magic_box evaluates to 1); this
    branch stays VALUE ONLY on every learner -- the DiCE gradient exists in the fused calls alone (fast_adapt_vpg(dice=True))."""
    episodes = _as_replay(episodes)
    adv = compute_advantages(baseline, tau, gamma, episodes['rewards'], episodes['dones'], episodes['states'], episodes['next_states'])
    adv_t = torch.from_numpy(adv).to(device=device, dtype=torch.float32)
    if dice:
        return -adv_t.mean()
    stepwise = hasattr(learner, 'fast_weights') and hasattr(_unwrap(learner), 'flat_parameters')
    lp = (learner if stepwise else _unwrap(learner)).log_prob(episodes['states'].to(device), episodes['actions'].to(device))
    return -(lp * adv_t).mean()


def fast_adapt_ppo(task, learner, baseline, params, anil=False, render=False):
    """reference rl.py:267-318: ppo_epochs clipped-surrogate updates per adapt step (second order, as learner.adapt defaults)."""
    return _adapt_task_walk(task, learner, baseline, params, 'ppo', anil, False)


def single_ppo_update(episodes, learner, baseline, params, anil=False):
    """reference rl.py:319-336: ONE clipped-surrogate update of the learner on ``episodes`` (normalised advantages, the baseline
    re-fitted, old log-probabilities at the learner's current parameters) through mi_policy_update with tasks = 1.  The learner's
    parameters are updated in place -- step size ``learner.lr`` (the MAML wrapper's, as ``learner.adapt`` uses it) or
    ``params['inner_lr']`` -- and the loss before the update is returned.  As in ``trpo_update``, ``anil`` only allows unused
    parameters (rl.py:335); whether the body moves is the policy's own switch (``turn_off_body_grads``)."""
    pol = _unwrap(learner)
    b = _replay_batch([_as_replay(episodes)], pol.input_size, pol.output_size, pol.sigma.device)
    b['adv'], _ = _batch_advantages(b, baseline, params['gamma'], params['tau'])
    lr = learner.lr if isinstance(getattr(learner, 'lr', None), (int, float)) else params['inner_lr']
    theta, loss = pol.engine().update(pol.flat(), b['states'], b['actions'], b['adv'], b['count'], lr, loss='ppo', epochs=1,
                                      clip=params.get('ppo_clip_ratio', 0.1), head_only=bool(getattr(pol, 'features_no_grad', False)))
    pol.load_flat(theta[0].contiguous())
    return loss[0, 0]


class AdaptedTasks:
    """What ``fast_adapt_vpg_tasks`` / ``fast_adapt_ppo_tasks`` return for the T tasks of a call: ``total_loss`` (0-dim, the sum of
    the validation losses; ``.backward()`` accumulates the summed meta-gradient), ``valid_loss [T]``, ``reward [T]``, ``success [T]``,
    ``theta [T, P]`` (the adapted parameters the query was rolled out with) and ``replays`` (per task the adapt_steps + 1 ``Replay``
    views, or None)."""
    __slots__ = ('total_loss', 'valid_loss', 'reward', 'success', 'theta', 'replays')

    def __init__(self, total_loss, valid_loss, reward, success, theta, replays):
        self.total_loss, self.valid_loss, self.reward, self.success = total_loss, valid_loss, reward, success
        self.theta, self.replays = theta, replays


def _task_rollout_ids(first_id, tasks, adapt_steps, stride=None):
    """ids[k][i]: the rollout id of run k (support steps, then the query) of task i: ``first_id + i * stride + k``,
    stride = adapt_steps + 1 unless the caller reserves further runs per task."""
    stride = adapt_steps + 1 if stride is None else stride
    return [[first_id + i * stride + k for i in range(tasks)] for k in range(adapt_steps + 1)]


def _adapt_tasks(goals, policy, baseline, params, seed, first_id, algo, anil, first_order, dice, want_replays, stride=None):
    """``_adapt_and_validate`` for all tasks on device rollouts -> ``AdaptedTasks``."""
    pol = _unwrap(policy)
    T, run = _rollout_run('fast_adapt_ppo_tasks' if algo == 'ppo' else 'fast_adapt_vpg_tasks', pol, goals, params, seed, first_id, stride)
    total, lt, theta, qry, replays = _adapt_and_validate(run, pol, baseline, params, algo, anil, first_order, dice, want_replays, learner=policy)
    thetas = theta if theta.dim() == 2 else theta.unsqueeze(0).expand(T, -1)
    reward = qry['rewards'].sum(dim=1) / params['adapt_batch_size']
    # the device rollout records no success signal: what get_ep_successes counts for such replays (rl.py:69-71)
    success = torch.zeros(T, device=pol.sigma.device)
    return AdaptedTasks(total, lt, reward, success, thetas, replays)


def fast_adapt_vpg_tasks(goals, policy, baseline, params, seed, first_id, anil=False, first_order=False, dice=False, want_replays=True):
    """``fast_adapt_vpg`` (reference rl.py:231-255) for ALL tasks of a meta-batch at once on device rollouts.  Per adapt step: one
    rollout call with the tasks' current parameters, one mi_gae_advantages launch (not normalised) and one mi_policy_update call
    over all tasks; then the query rollout, its advantages, and ONE mi_policy_meta_batch call from the shared parameters over all
    support batches and the query, which returns the validation losses and the meta-gradient summed over tasks.  Task i's run k
    uses rollout id ``first_id + i * (adapt_steps + 1) + k`` -- what it gets from ``fast_adapt_vpg`` with
    ``Particles2DRunner(goal, L, rollout='device', seed=seed, first_id=first_id + i * (adapt_steps + 1))``.  Returns an
    ``AdaptedTasks`` record.  With ``want_replays=False`` nothing is read back from the device during the call; otherwise the row
    counts are read once per rollout.  ``baseline`` is left as after the task-by-task walk: fitted to the last task's query replay."""
    return _adapt_tasks(goals, policy, baseline, params, seed, first_id, 'vpg', anil, first_order, dice, want_replays)


def fast_adapt_ppo_tasks(goals, policy, baseline, params, seed, first_id, anil=False, want_replays=True):
    """``fast_adapt_ppo`` (reference rl.py:267-318) for ALL tasks of a meta-batch at once: as ``fast_adapt_vpg_tasks`` with normalised
    advantages and ``ppo_epochs`` clipped-surrogate updates per adapt step in one mi_policy_update call (old log-probabilities
    taken once per step, at the parameters the step starts from); second order, as ``learner.adapt`` defaults."""
    return _adapt_tasks(goals, policy, baseline, params, seed, first_id, 'ppo', anil, False, False, want_replays)


def _eval_tasks(env, params, goals):
    """The evaluation tasks and a runner factory for them.  ``env`` as the reference passes it (rl.py:142-196: an environment NAME handed to
    make_env, whose result offers ``sample_tasks / set_task / reset``): 'Particles2D-v1' (or any name containing 'Particles2D') builds this
    package's ``Particles2DEnv``; an env-like object is used as it is -- ``Particles2DEnv`` through the device-vectorised
    ``Particles2DRunner``, anything else through the host loop of ``EnvRunner``; a sequence of goals (this package's earlier signature, also
    the ``goals=`` keyword) is taken as the task list itself."""
    if goals is None and not isinstance(env, str) and not hasattr(env, 'sample_tasks'):
        goals, env = env, None
    if isinstance(env, str):
        if 'Particles2D' not in env:
            raise NotImplementedError(f'environment {env!r}: this package ships Particles2D (Meta-World / MuJoCo are out of scope); pass an '
                                      'env-like object with sample_tasks / set_task / reset / step instead of a name')
        env = Particles2DEnv(seed=params.get('seed', 42))
    if goals is not None:
        tasks = [{'goal': g} for g in goals]
        env = env if env is not None else Particles2DEnv(seed=params.get('seed', 42))
    else:
        tasks = env.sample_tasks(params['n_tasks'])                                    # rl.py:162
    return env, tasks


def _evaluate_device(algo, env, tasks, policy, baseline, params, anil, seed, first_id):
    """evaluate() with every run on the device and all tasks per call: task i owns the rollout ids ``first_id + i * (adapt_steps + 2)
    + k``, k = 0 .. adapt_steps for the adaptation (support steps, query) and adapt_steps + 1 for the final episodes -- the ids of
    ``Particles2DRunner(goal, L, rollout='device', seed=seed, first_id=first_id + i * (adapt_steps + 2))`` walked as below."""
    if not isinstance(env, Particles2DEnv):
        raise NotImplementedError("evaluate(rollout='device') rolls out Particles2D; other environments take the host loop")
    if algo not in ('vpg', 'ppo'):
        raise NotImplementedError("evaluate(rollout='device') adapts with 'vpg' or 'ppo' (fast_adapt_vpg_tasks / fast_adapt_ppo_tasks)")
    goals = np.asarray([t['goal'] for t in tasks], dtype=np.float32).reshape(-1, 2)
    K, E, L = params['adapt_steps'], params['adapt_batch_size'], params['max_path_length']
    with torch.no_grad():                                      # (fast_adapt_ppo is called without anil in evaluate, as below)
        res = _adapt_tasks(goals, policy, baseline, params, seed, first_id, algo, anil and algo == 'vpg', False, False, False, stride=K + 2)
    eng = _unwrap(policy).engine()
    out = eng.rollout(res.theta.contiguous(), goals, [first_id + i * (K + 2) + K + 1 for i in range(len(tasks))], seed, E, L)
    return (out['rewards'].sum(dim=1) / E).tolist(), [0.0] * len(tasks)


def evaluate(algo, env, policy, baseline, params, anil=False, render=False, generator=None, goals=None, rollout='host', first_id=0):
    """reference rl.py:142-196: adapt a copy of the policy to every evaluation task with `algo` in {'vpg', 'ppo', 'trpo'}, then roll out
    `adapt_batch_size` query episodes with the adapted policy.  ``env``: see ``_eval_tasks`` (name, env-like, or the task goals).
    ``rollout='device'`` ('vpg' / 'ppo' on Particles2D): all tasks are adapted and rolled out together through the batched
    functions, noise from ``(params['seed'], first_id + ...)`` (``_evaluate_device``); the default is the task-by-task host walk.
    Returns (tasks_rewards, mean reward, mean success rate)."""
    if rollout not in ('host', 'device'):
        raise ValueError("rollout must be 'host' or 'device'")
    env, tasks = _eval_tasks(env, params, goals)
    if rollout == 'device':
        tasks_rewards, tasks_success = _evaluate_device(algo, env, tasks, policy, baseline, params, anil, params.get('seed', 42), first_id)
        n = params.get('n_tasks', len(tasks_rewards))
        if isinstance(n, str):
            n = len(tasks_rewards)
        return tasks_rewards, sum(tasks_rewards) / n, sum(tasks_success) / n
    dev = _unwrap(policy).sigma.device
    tasks_rewards, tasks_success = [], []
    for task_desc in tasks:
        learner = deepcopy(policy)
        env.set_task(task_desc)                                                        # rl.py:166-167
        env.reset()
        if isinstance(env, Particles2DEnv):
            task = Particles2DRunner(env.goal, params['max_path_length'], generator, dev)
        else:
            task = EnvRunner(env, params['max_path_length'], dev)
        with torch.no_grad():
            if algo == 'vpg':
                fast_adapt_vpg(task, learner, baseline, params, anil=anil)
                adapted = learner._adapted_policy
            elif algo == 'ppo':
                fast_adapt_ppo(task, learner, baseline, params)
                adapted = learner._adapted_policy
            else:
                # (a wrapper with a fixed step-size table adapts with it; any other learner as the bare policy, as before)
                actor = learner if _trpo_lr_table(learner, 'evaluate_trpo') is not None else _unwrap(learner)
                adapted, _, _, _, _ = fast_adapt_trpo(task, actor, baseline, params, anil=anil)
        query = _as_replay(task.run(adapted, episodes=params['adapt_batch_size']))    # rl.py:181-184
        tasks_rewards.append(query['rewards'].sum().item() / params['adapt_batch_size'])
        tasks_success.append(get_ep_successes(query, params.get('max_path_length')) / params['adapt_batch_size'])
    n = params.get('n_tasks', len(tasks_rewards))
    if isinstance(n, str):                                                             # (rl.py:158-159: an explicit task name)
        n = len(tasks_rewards)
    return tasks_rewards, sum(tasks_rewards) / n, sum(tasks_success) / n


def evaluate_vpg(env, policy, baseline, eval_params, anil=False, render=False, generator=None, goals=None):
    """reference rl.py:258-259"""
    return evaluate('vpg', env, policy, baseline, eval_params, anil, render, generator, goals)


def evaluate_ppo(env, policy, baseline, eval_params, anil=False, render=False, generator=None, goals=None):
    """reference rl.py:340-341"""
    return evaluate('ppo', env, policy, baseline, eval_params, anil, render, generator, goals)


def evaluate_trpo(env, policy, baseline, eval_params, anil=False, render=False, generator=None, goals=None):
    """reference rl.py:476-477"""
    return evaluate('trpo', env, policy, baseline, eval_params, anil, render, generator, goals)


# ---------------------------------------------------------------------------------------------- Particles2D rollouts
class Particles2DRunner:
    """Minimal stand-in for core_functions/runner.py + learn2learn's Particles2D (both out of scope); ``run``
    returns a replay dict with episodes concatenated.  ``rollout='host'`` (default; host loop, device math): all ``episodes`` of a
    task advance in lock-step on the device, one step per pass of a Python loop, the noise from ``generator``.  ``rollout='device'``:
    the whole run is one mi_particles_rollout call and one read-back of the row count; the n-th ``run`` of
    this runner draws its noise from ``(seed, first_id + n)``, the generator is not used."""

    def __init__(self, goal, max_path_length, generator=None, dev=None, rollout='host', seed=0, first_id=0):
        self.dev = dev or device
        self.goal = torch.as_tensor(goal, dtype=torch.float32, device=self.dev)
        self.max_path_length, self.generator = max_path_length, generator
        if rollout not in ('host', 'device'):
            raise ValueError("rollout must be 'host' or 'device'")
        self.rollout, self.seed, self.first_id, self.runs = rollout, int(seed), int(first_id), 0

    def _run_device(self, policy, episodes):
        pol = _unwrap(policy)
        out = pol.engine().rollout(pol.flat(), self.goal.reshape(1, 2), [self.first_id + self.runs], self.seed, episodes, self.max_path_length)
        self.runs += 1
        return _replay_rows(out, 0, int(out['count'].item()))

    def run(self, policy, episodes):
        if self.rollout == 'device':
            return self._run_device(policy, episodes)
        E, L = episodes, self.max_path_length
        state = torch.zeros(E, 2, device=self.dev)
        active = torch.ones(E, dtype=torch.bool, device=self.dev)
        S, A, R, D, NS, M = [], [], [], [], [], []
        scale = torch.exp(torch.clamp(policy.sigma.detach(), min=np.log(1e-6)))
        theta, eng = policy.flat(), policy.engine()
        for t in range(L):
            loc = eng.forward(theta, state.unsqueeze(0))[0]
            action = loc + scale * torch.randn(loc.shape, device=self.dev, generator=self.generator)
            nxt = state + action.clamp(-0.1, 0.1)
            diff = nxt - self.goal
            reward = -diff.norm(dim=1)
            done = (diff.abs() < 0.01).all(dim=1)
            last = done | (t == L - 1)
            S.append(state); A.append(action); R.append(reward); D.append(last.float()); NS.append(nxt); M.append(active)
            state = nxt
            active = active & ~done
        S, A, NS = torch.stack(S, 1), torch.stack(A, 1), torch.stack(NS, 1)          # [E, L, *]
        R, D, M = torch.stack(R, 1), torch.stack(D, 1), torch.stack(M, 1)
        keep = M.reshape(-1)
        flat = lambda x: x.reshape(E * L, -1)[keep]
        return Replay(states=flat(S), actions=flat(A), rewards=flat(R), dones=flat(D), next_states=flat(NS))


class Particles2DEnv:
    """learn2learn's Particles2D as the reference's drivers use it (rl/maml_trpo.py:100-108: ``sample_tasks / set_task / reset``; out of
    scope as a dependency): state in R^2 from the origin, goal ~ U(-0.5, 0.5)^2, action clipped to +-0.1,
    reward = -||state - goal||_2, done when both |state - goal| < 0.01.  Episodes are rolled out on the device by ``Particles2DRunner``
    (``runner()``); ``step`` is the same arithmetic one step at a time on the host, for callers that drive the env themselves."""
    state_size, action_size = 2, 2

    def __init__(self, seed=42):
        self.rng = np.random.RandomState(seed)
        self.goal = np.zeros(2, dtype=np.float32)
        self.state = np.zeros(2, dtype=np.float32)

    def sample_tasks(self, num_tasks):
        return [{'goal': g} for g in self.rng.uniform(-0.5, 0.5, size=(num_tasks, 2))]

    def set_task(self, task):
        self.goal = np.asarray(task['goal'], dtype=np.float32)

    def reset(self):
        self.state = np.zeros(2, dtype=np.float32)
        return self.state.copy()

    def step(self, action):
        self.state = self.state + np.clip(np.asarray(action, dtype=np.float32).reshape(2), -0.1, 0.1)
        diff = self.state - self.goal
        return self.state.copy(), -float(np.sqrt((diff * diff).sum())), bool((np.abs(diff) < 0.01).all()), {}

    def runner(self, max_path_length, generator=None, dev=None, rollout='host', seed=0, first_id=0):
        return Particles2DRunner(self.goal, max_path_length, generator, dev, rollout, seed, first_id)


class EnvRunner:
    """``task.run(policy, episodes=n)`` for ANY env-like object (``reset() -> state``, ``step(action) -> (state, reward, done, info)``):
    the host loop of the reference's core_functions/runner.py for one environment, the policy evaluated on the device one state at a
    time.  ``info['success']`` (Meta-World's signal, runner.py's ``extra_info``) is recorded as the replay's ``success`` when present.
    Slow by construction (an environment step per policy call); Particles2D has its own vectorised runner."""

    def __init__(self, env, max_path_length, dev=None):
        self.env, self.max_path_length, self.dev = env, max_path_length, dev or device

    def run(self, policy, episodes, render=False):
        S, A, R, D, NS, SU = [], [], [], [], [], []
        any_success = False
        for _ in range(episodes):
            state = np.asarray(self.env.reset(), dtype=np.float32).reshape(-1)
            for t in range(self.max_path_length):
                st = torch.from_numpy(state).to(self.dev).reshape(1, -1)
                action = policy(st)[0]
                nxt, reward, done, info = self.env.step(action.detach().cpu().numpy())
                nxt = np.asarray(nxt, dtype=np.float32).reshape(-1)
                last = bool(done) or t == self.max_path_length - 1
                S.append(st[0]); A.append(action.detach().float()); R.append(float(reward)); D.append(1.0 if last else 0.0)
                NS.append(torch.from_numpy(nxt).to(self.dev))
                if isinstance(info, dict) and 'success' in info:
                    any_success = True
                    SU.append(float(info['success']))
                else:
                    SU.append(0.0)
                state = nxt
                if done:
                    break
        col = lambda x: torch.tensor(x, dtype=torch.float32, device=self.dev).reshape(-1, 1)
        out = Replay(states=torch.stack(S).contiguous(), actions=torch.stack(A).contiguous(), rewards=col(R), dones=col(D),
                     next_states=torch.stack(NS).contiguous())
        if any_success:
            out['success'] = col(SU)
        return out
