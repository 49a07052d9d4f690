"""Cases of tests/test_gpu_trpo_parity.py: the TRPO entry points against what the commit before their unification computed.

Until then meta_surrogate_loss, its gradient and the two curvature products existed twice in csrc/policy.hip: once for a single inner
update (mi_trpo_surrogate / _fvp / _kl_prepare / _fvp_general, fused sweeps or per-layer launches) and once for K updates (the *_steps
entry points).  The K-step path is now the only one.  tests/golden/trpo_parity_parent.npz holds the inputs of every case and the
outputs of that earlier build, through the route the case names; tools/record_trpo_parity.py wrote it from a build of the earlier
commit, never from the code under test.

A case is a function of an adapter with four callables -- surrogate, fvp, kl_prepare, fvp_general, with PolicyEngine's argument lists
-- and of its inputs; it returns the named outputs.  The test passes a PolicyEngine; the recorder passes, for the `one_step` route, a
wrapper of the earlier library's one-step symbols."""
import os
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'trpo_parity_parent.npz')
DAMPING = 1e-5
KEYS = ('states', 'actions', 'adv', 'count')

# input set -> (S, A, hiddens, activation).  The four 2-100-100-2 sets share theta, the directions and the displaced candidate.
SETS = OrderedDict([
    ('relu', (2, 2, (100, 100), 'relu')),              # test_gpu_rl._replays(): old = the adapted policy
    ('relu_anil', (2, 2, (100, 100), 'relu')),         # old policies adapted head-only
    ('tanh_anil', (2, 2, (100, 100), 'tanh')),         # test_gpu_rl._replays_tanh(anil=True)
    ('tanh_k2', (2, 2, (100, 100), 'tanh')),           # test_gpu_anil_trpo_steps._case('tanh', 2, 0.1): two inner updates
    ('odd', (3, 1, (5, 3), 'tanh')),                   # policy_shapes_oracle 'odd_5x3': odd widths, A = 1, a task with one valid row
])
SHARED = ('theta', 'v', 'cand')


def _set_fused(on):
    from exploring_meta_amd import _lib
    _lib.load().mi_policy_set_fused_fvp(int(on))


def _surrogate(a, x, theta, want_grad):
    return a.surrogate(theta, x.sup, x.qry, x.old_loc, x.old_scale, x.lr, want_grad)


def _values_and_gradient(a, x, out):
    """loss, KL, gradient at theta; loss / KL at the displaced candidate (the line search's call); then back at theta, whose passes the
    products read."""
    loss, kl, grad = _surrogate(a, x, x.theta, True)
    out.update(loss=loss, kl=kl, grad=grad)
    out['cand_loss'], out['cand_kl'], _ = _surrogate(a, x, x.cand, False)
    _surrogate(a, x, x.theta, True)


def fisher(a, x, dirs=(0,), fused=1, ragged=False):
    """MAML-TRPO: surrogate, gradient and the Fisher form of the product."""
    if ragged:                                   # tasks 0 and 2 lose rows: everything behind count is padding to every kernel
        x = SimpleNamespace(**vars(x))
        x.sup, x.qry = dict(x.sup), dict(x.qry)
        for d, row in ((x.sup, lambda c: c[0]), (x.qry, lambda c: c)):
            c = d['count'].clone()
            row(c)[0], row(c)[2] = 97, 33
            d['count'] = c.contiguous()
    out = OrderedDict()
    _set_fused(fused)
    try:
        _values_and_gradient(a, x, out)
        for i in dirs:
            out[f'fvp{i}'] = a.fvp(x.sup, x.qry, x.lr, DAMPING, x.v[i])
        torch.cuda.synchronize()
    finally:
        _set_fused(1)
    return out


def general(a, x, dirs=(0,), fisher_product=True, values=True, grad=True, kl_grad=True):
    """ANIL-TRPO: the surrogate, then the exact Hessian of the mean KL (and, first, the Fisher form on the same passes)."""
    out = OrderedDict()
    if values:
        _values_and_gradient(a, x, out)
    else:
        out['loss'], out['kl'], g = _surrogate(a, x, x.theta, True)
        if grad:
            out['grad'] = g
    if fisher_product:
        out['fvp0'] = a.fvp(x.sup, x.qry, x.lr, DAMPING, x.v[0])
    g = a.kl_prepare(x.sup, x.qry, x.old_loc, x.old_scale, x.lr, want_grad=kl_grad)
    if kl_grad:
        out['kl_grad'] = g
    for i in dirs:
        out[f'fvp_general{i}'] = a.fvp_general(x.sup, x.qry, x.old_scale, x.lr, DAMPING, x.v[i])
    torch.cuda.synchronize()
    return out


# case -> (input set, route in the earlier build, bar, function, its keywords).  `bitwise`: the earlier kernels with the earlier
# arguments at other addresses; `close`: the K-step per-layer kernels against the one-step ones (gauss2_kernel against gauss_kernel).
CASES = OrderedDict([
    ('a_relu_fused', ('relu', 'one_step', 'bitwise', fisher, dict(dirs=(0,)))),
    ('b_relu_fused_ragged', ('relu', 'one_step', 'bitwise', fisher, dict(dirs=(0,), ragged=True))),
    ('c_relu_per_layer', ('relu', 'one_step', 'close', fisher, dict(dirs=(0,), fused=0))),
    ('d_tanh_general', ('tanh_anil', 'one_step', 'close', general, dict())),
    ('e_relu_fused_general', ('relu_anil', 'one_step', 'close', general, dict(dirs=(0, 1), fisher_product=False, values=False, grad=False))),
    ('f_odd_tanh_general', ('odd', 'one_step', 'close', general, dict())),
    ('g_tanh_two_steps', ('tanh_k2', 'steps', 'bitwise', general, dict(values=False))),
    ('h_tanh_two_steps_no_kl_grad', ('tanh_k2', 'steps', 'bitwise', general, dict(dirs=(0, 1), fisher_product=False, values=False,
                                                                                 grad=False, kl_grad=False))),
])
SCALARS = ('loss', 'kl', 'cand_loss', 'cand_kl')


def general_case(case):
    return CASES[case][3] is general


def load_inputs(npz, name, device='cuda'):
    """The inputs of an input set from the fixture, on the device."""
    def get(key):
        k = f'{name}/{key}'
        return torch.from_numpy(npz[k if k in npz.files else key]).to(device).contiguous()
    x = SimpleNamespace(theta=get('theta'), v=get('v'), cand=get('cand'), old_loc=get('old_loc'), old_scale=get('old_scale'),
                        lr=float(npz[f'{name}/lr']))
    x.sup = {k: get(f'sup_{k}') for k in KEYS}
    x.qry = {k: get(f'qry_{k}') for k in KEYS}
    return x


def expected(npz, case):
    return OrderedDict((k.split('/')[-1], npz[k]) for k in npz.files if k.startswith(f'{case}/out/'))


def engine(name):
    from exploring_meta_amd.engine import PolicyEngine
    S, A, H, act = SETS[name]
    return PolicyEngine(S, A, H, activation=act)


# --------------------------------------------------------------------------------------------------- the recorder's side
def build_inputs():
    """name -> arrays of every input set (numpy), from the oracle's replays through _SurrogateContext's padding.  Recorder only: needs
    the oracle and the GPU; the test reads the fixture."""
    from exploring_meta_amd import core_functions as cf
    from exploring_meta_amd.core_functions.rl import _SurrogateContext
    from oracle import rl_ref as RL
    import policy_shapes_oracle as PO
    from test_gpu_rl import PARAMS, _replays, _replays_tanh, _policy, _policy_tanh, _theta64
    from test_gpu_anil_trpo_steps import _case
    arrays = {}

    def put(name, sup, qry, old_loc, old_scale, lr):
        for k in KEYS:
            arrays[f'{name}/sup_{k}'], arrays[f'{name}/qry_{k}'] = sup[k].cpu().numpy(), qry[k].cpu().numpy()
        arrays[f'{name}/old_loc'], arrays[f'{name}/old_scale'] = old_loc.cpu().numpy(), old_scale.cpu().numpy()
        arrays[f'{name}/lr'] = np.float64(lr)

    def from_context(name, params, theta, replays, olds, mk):
        ctx = _SurrogateContext(replays, [mk(o) for o in olds], mk(theta), cf.LinearValue(2, 2), params)
        put(name, ctx.sup, ctx.qry, ctx.old_loc, ctx.old_scale, ctx.inner_lr)
        return mk(theta).flat()

    theta, replays, olds = _replays()
    th = from_context('relu', PARAMS, theta, replays, olds, _policy)
    env, gen, baseline = RL.Particles2D(seed=1), torch.Generator().manual_seed(2), RL.LinearValue(2, 2)
    replays, olds = [], []
    for task in env.sample_tasks(PARAMS['meta_batch_size']):           # ReLU body, old policies adapted head-only
        env.set_task(task)
        learner = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in _theta64().items())
        adapted, _, rep, _ = RL.fast_adapt_trpo(env, learner, baseline, PARAMS, gen, first_order=True, anil=True)
        replays.append(rep)
        olds.append(OrderedDict((k, v.detach()) for k, v in adapted.items()))
    from_context('relu_anil', PARAMS, _theta64(), replays, olds, _policy)
    theta, replays, olds = _replays_tanh(anil=True)
    from_context('tanh_anil', PARAMS, theta, replays, olds, _policy_tanh)
    P2, _, theta, replays, olds = _case('tanh', 2, 0.1)
    from_context('tanh_k2', P2, theta, replays, olds, _policy_tanh)
    g = torch.Generator().manual_seed(5)
    arrays['theta'] = th.cpu().numpy()
    arrays['v'] = torch.randn(2, th.numel(), generator=g, dtype=torch.float64).float().numpy()
    arrays['cand'] = (th + 0.01 * torch.sin(torch.arange(th.numel(), device=th.device, dtype=torch.float32))).cpu().numpy()

    inp, ref, _ = PO.reference('odd_5x3')
    r = ref['trpo', 1, 'general']
    f = lambda t: torch.as_tensor(t).float()
    sup = {k: (inp['sup'][k][:1].to(torch.int32) if k == 'count' else f(inp['sup'][k][:1])) for k in KEYS}
    qry = {k: (inp['qry'][k].to(torch.int32) if k == 'count' else f(inp['qry'][k])) for k in KEYS}
    put('odd', sup, qry, f(r['old_loc']), f(r['old_scale']), PO.INNER_LR)
    arrays['odd/theta'], arrays['odd/cand'] = f(inp['theta']).numpy(), f(inp['cand']).numpy()
    arrays['odd/v'] = torch.stack([f(v) for v in r['v']]).numpy()
    return arrays
