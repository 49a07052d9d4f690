"""Per-parameter inner-loop step sizes of the policy's fused calls, the parts that need no GPU:
(a) the recursion the kernels implement (tests/policy_lr_oracle.py::closed_form) against fp64 autograd at 1e-12 -- the bar of
    tests/test_inner_lr_host.py for the vision recursion -- on a 3-5-4-2 policy with two tasks;
(b) ``MAML.lr_flat()`` around a policy: the ENGINE's parameter order (sigma first) -- the registration order of the two shipped policy
    classes, and a gather for a policy registered otherwise --, frozen tensors, gradients back to ``InnerLR.values``, and the mapping of
    adapt steps to rows of the step-size table;
and the argument checks of the new C entries, which run before any HIP call."""
import ctypes as C

import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as cf_rl
import policy_lr_oracle as O


def _inputs():
    # 3-5-4-2, T = 2, ragged counts, two support replays and the query
    return O.random_inputs(3, 2, (5, 4), 2, 9, [(9, 6), (7, 9), (9, 8)], seed=11)


CASES = {
    # name: (activation, kind, step_batch, step_lr_row, rows, head_only, first_order, frozen)
    'a2c_rows_per_update': ('tanh', 'a2c', [0, 1], [0, 1], 2, False, False, ()),
    'ppo_2x2_epochs_share_rows': ('tanh', 'ppo', [0, 0, 1, 1], [0, 0, 1, 1], 2, False, False, ()),
    'head_only': ('tanh', 'a2c', [0, 1], [0, 1], 2, True, False, ()),
    'first_order': ('tanh', 'a2c', [0, 1], [0, 1], 2, False, True, ()),
    'one_tensor_frozen': ('tanh', 'a2c', [0, 1], None, 1, False, False, ('mean.0.',)),
    'dice_relu': ('relu', 'dice', [0, 1], [0, 1], 2, False, False, ('mean.2.',)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_closed_form_is_fp64_autograd(name):
    act, kind, step_batch, step_lr_row, rows, head_only, fo, frozen = CASES[name]
    inp = _inputs()
    o = O.Oracle(inp['S'], inp['A'], inp['H'], act)
    lr = O.lr_vector(o, 0.3, rows, 7, frozen=frozen)
    args = (inp['theta'], inp['sup'], inp['qry'], step_batch, lr, step_lr_row)
    kw = dict(kind=kind, clip=0.1, head_only=head_only, first_order=fo)
    want = o.meta_lr(*args, **kw)
    got = O.closed_form(o, *args, **kw)
    for w, g, what in zip(want, got, ('loss', 'theta_out', 'grad', 'lr_grad')):
        scale = max(1.0, float(w.abs().max()))
        assert float((w - g).abs().max()) <= 1e-12 * scale, (name, what, float((w - g).abs().max()))
    lr_grad, fm = want[3], O.frozen_mask(o, frozen)
    assert float(lr_grad.abs().max()) > 0
    if frozen:                                                   # frozen, not detached: the step's gradient is alive there
        assert float(lr_grad[:, fm].abs().max()) > 0
        assert torch.equal(want[1][:, fm], inp['theta'][fm].expand(inp['T'], -1))
    if head_only:
        body = o.head_mask() == 0
        assert torch.equal(lr_grad[:, body], torch.zeros_like(lr_grad[:, body]))
        assert torch.equal(want[1][:, body], inp['theta'][body].expand(inp['T'], -1))


def test_update_is_the_forward_half_of_the_fused_call():
    inp = _inputs()
    o = O.Oracle(inp['S'], inp['A'], inp['H'], 'tanh')
    lr = O.lr_vector(o, 0.3, 1, 7)
    s0 = {k: v[0] for k, v in inp['sup'].items()}
    for kind, epochs in (('a2c', 1), ('ppo', 3)):
        want = o.meta_lr(inp['theta'], inp['sup'], inp['qry'], [0] * epochs, lr, kind=kind)[1]
        assert float((o.update_lr(inp['theta'], s0, lr[0], kind=kind, epochs=epochs) - want).abs().max()) <= 1e-14


# ------------------------------------------------------------------------------------------------------------- (b)
class _SigmaInChild(torch.nn.Module):
    """A policy (the protocol ``MAML`` looks for: ``density``, ``flat_parameters``, ``_engine_params``) whose registration order is NOT the
    engine's: ``sigma`` sits in a child module registered after the layers, so ``named_parameters()`` ends with it while
    ``_engine_params()`` starts with it.  The two shipped classes register ``sigma`` on the module itself, which ``named_parameters()``
    lists before any child's parameters: their two orders agree and ``_engine_order`` moves nothing."""

    def __init__(self):
        super().__init__()
        lin = torch.nn.Linear
        self.mean = torch.nn.Sequential(lin(3, 5), torch.nn.Tanh(), lin(5, 4), torch.nn.Tanh(), lin(4, 2))
        self.noise = torch.nn.Module()
        self.noise.sigma = torch.nn.Parameter(torch.zeros(2))

    def _engine_params(self):
        return [self.noise.sigma] + [q for m in self.mean if isinstance(m, torch.nn.Linear) for q in (m.weight, m.bias)]

    def flat_parameters(self):
        return torch.cat([q.reshape(-1) for q in self._engine_params()])

    def density(self, state, theta=None):
        raise NotImplementedError('order test only')


def _policies():
    return [('DiagNormalPolicy', cf.DiagNormalPolicy(3, 2, hiddens=[5, 4], activation='tanh'), 'mean.0.'),
            ('DiagNormalPolicyANIL', cf.DiagNormalPolicyANIL(3, 2, 4, hiddens=[5, 4]), 'body.0.'),
            ('sigma_in_child', _SigmaInChild(), 'mean.0.')]


@pytest.mark.parametrize('which', [0, 1, 2])
def test_lr_flat_follows_the_engine_order(which):
    """Index-valued steps: entry j of ``values`` (named_parameters() order) must sit where the engine keeps that parameter.  For the two
    shipped classes the orders agree (asserted); 'sigma_in_child' is the case in which they do not, and the one that exercises the gather of
    ``MAML._engine_order``: values, frozen slots and the routing of gradients back to ``InnerLR.values``."""
    name, pol, prefix = _policies()[which]
    moved = [id(q) for q in pol.parameters()] != [id(q) for q in pol._engine_params()]
    assert moved == (name == 'sigma_in_child')
    P = sum(q.numel() for q in pol.parameters())
    init = torch.arange(1, 2 * P + 1, dtype=torch.float32).reshape(2, P)
    lr = cf.InnerLR(pol, init, per='parameter', steps=2, learnable=True, frozen=(prefix,))
    maml = cf.MAML(pol, lr=lr)
    flat = maml.lr_flat()
    assert tuple(flat.shape) == (2, P)
    start, off = {}, 0
    for n, q in pol.named_parameters():
        start[id(q)] = (off, n)
        off += q.numel()
    want, frozen = [], []
    for q in pol._engine_params():
        o, n = start[id(q)]
        want += list(range(o, o + q.numel()))
        frozen += [n.startswith(prefix)] * q.numel()
    want, frozen = torch.tensor(want), torch.tensor(frozen)
    assert start[id(pol._engine_params()[0])][1].endswith('sigma') and frozen.sum() == 3 * 5 + 5 and not frozen[:2].any()
    for r in range(2):
        expect = torch.where(frozen, torch.zeros(P), init[r][want])
        assert torch.equal(flat[r].detach(), expect), name
    # gradients sent back through lr_flat() land on the entries they belong to; none reaches a frozen slot
    w = torch.arange(1, 2 * P + 1, dtype=torch.float32).reshape(2, P) * 0.5
    (flat * w).sum().backward()
    g = lr.values.grad
    expect = torch.zeros(2, P)
    for r in range(2):
        expect[r][want[~frozen]] = w[r][~frozen]
    assert torch.equal(g, expect), name
    # the step-wise learner's rows: engine order too
    assert torch.equal(maml._step_lr().detach(), flat[0].detach())
    # per='tensor': a tensor's step lands on all its engine slots
    lt = cf.InnerLR(pol, torch.arange(1, 8, dtype=torch.float32).reshape(1, 7), per='tensor')
    ft = cf.MAML(pol, lr=lt).lr_flat()[0]
    names = [n for n, _ in pol.named_parameters()]
    off = 0
    for q in pol._engine_params():
        j = names.index(start[id(q)][1])
        assert torch.equal(ft[off:off + q.numel()], torch.full((q.numel(),), float(j + 1))), (name, names[j])
        off += q.numel()
    assert cf.MAML(pol, lr=0.1).lr_flat() is None


def test_adapt_steps_map_to_rows_or_raise():
    assert cf_rl._lr_step_rows(1, 3) == [0, 0, 0]
    assert cf_rl._lr_step_rows(3, 3) == [0, 1, 2]
    assert cf_rl._lr_step_rows(1, 1) == [0]
    for rows, steps in ((2, 3), (3, 2), (4, 1)):
        with pytest.raises(ValueError, match='adapt_steps'):
            cf_rl._lr_step_rows(rows, steps)
    pol = _policies()[0][1]
    wrapped = cf.MAML(pol, lr=cf.InnerLR(pol, 0.1, per='tensor', steps=3))
    assert cf_rl._policy_lr_vector(wrapped).shape[0] == 3
    assert cf_rl._policy_lr_vector(cf.MAML(pol, lr=0.1)) is None and cf_rl._policy_lr_vector(pol) is None
    for name in ('fast_adapt_trpo', 'meta_optimize_trpo'):
        with pytest.raises(ValueError, match=name):
            cf_rl._refuse_lr_vector(wrapped, name)
    cf_rl._refuse_lr_vector(cf.MAML(pol, lr=0.1), 'meta_optimize_trpo')


def test_driver_flags_build_the_wrapper_lr():
    from exploring_meta_amd.rl import maml_ppo
    pol = _policies()[0][1]
    p = dict(maml_ppo.params)
    assert maml_ppo.inner_lr_of(pol, p) == p['inner_lr']
    lr = maml_ppo.inner_lr_of(pol, dict(p, adapt_steps=2, inner_lr_per='tensor', learn_inner_lr=True, per_step_lr=True, freeze=['mean.0.']))
    assert isinstance(lr, cf.InnerLR) and lr.learnable and lr.steps == 2 and lr.per == 'tensor' and lr.frozen == ('mean.0.',)
    assert any(q is lr.values for q in cf.MAML(pol, lr=lr).parameters())        # Adam(policy.parameters()) carries the step sizes


# ------------------------------------------------------------------------------------------------------------- C argument checks
def test_argument_errors_come_before_any_hip_call():
    """MI_ERR_ARG with a text naming the entry and the value; no device is touched (this runs without one: the pointers are host
    addresses the library must not follow)."""
    lib = _lib.load()
    desc = _lib.MiPolicyDesc(2, 2, 100, 100, 0)
    h = C.c_void_p()
    assert lib.mi_policy_create(C.byref(desc), 0, C.byref(h)) == 0
    ptr = C.c_void_p(64)
    one = (C.c_int32 * 2)(0, 0)
    rows = (C.c_int32 * 2)(0, 2)

    def meta(lr_vec=ptr, lr_rows=1, step_lr_row=None, with_grad=1, lr_grad=None, steps=2):
        return lib.mi_policy_meta_batch_lr(h, None, ptr, steps, one, one, step_lr_row, 1, ptr, ptr, ptr, None, None, ptr, ptr, ptr, None, None,
                                           2, 4, 0, 0.1, lr_vec, lr_rows, 0, 1, with_grad, ptr, ptr, ptr, lr_grad, ptr, 1 << 30)
    for call, text in ((lambda: meta(lr_vec=None), b'lr_vec'), (lambda: meta(lr_rows=0), b'lr_rows 0'), (lambda: meta(lr_rows=65536), b'lr_rows 65536'),
                       (lambda: meta(lr_rows=2, step_lr_row=rows), b'step_lr_row[1] 2'),
                       (lambda: meta(with_grad=0, lr_grad=ptr), b'lr_grad_out'), (lambda: meta(steps=257), b'steps 257')):
        assert call() == -1
        msg = lib.mi_policy_last_error(None)
        assert b'mi_policy_meta_batch_lr' in msg and text in msg, msg
    rc = lib.mi_policy_update_lr(h, None, ptr, 0, ptr, ptr, ptr, None, None, 2, 4, 0, 1, 0.1, None, 0, ptr, None, ptr, 1 << 30)
    assert rc == -1 and b'mi_policy_update_lr' in lib.mi_policy_last_error(None) and b'lr_vec' in lib.mi_policy_last_error(None)
    rc = lib.mi_policy_update_lr(h, None, ptr, 0, ptr, ptr, ptr, None, None, 2, 4, 0, 65, 0.1, ptr, 0, ptr, None, ptr, 1 << 30)
    assert rc == -1 and b'mi_policy_update_lr: epochs 65' in lib.mi_policy_last_error(None)
    n, m = C.c_size_t(), C.c_size_t()
    assert lib.mi_policy_meta_lr_workspace_bytes(h, 2, 4, 2, 1, 1, 0, 1, C.byref(n)) == -1
    assert lib.mi_policy_meta_lr_workspace_bytes(h, 2, 4, 2, 1, 1, 65536, 1, C.byref(n)) == -1
    assert lib.mi_policy_meta_lr_workspace_bytes(h, 2, 4, 2, 1, 1, 65535, 1, C.byref(n)) == 0
    assert lib.mi_policy_meta_workspace_bytes(h, 2, 4, 2, 1, 1, C.byref(m)) == 0
    assert lib.mi_policy_meta_lr_workspace_bytes(h, 2, 4, 2, 1, 1, 2, 0, C.byref(n)) == 0 and n.value == m.value
    assert lib.mi_policy_meta_lr_workspace_bytes(h, 2, 4, 2, 1, 1, 2, 1, C.byref(n)) == 0 and n.value > m.value
    lib.mi_policy_destroy(h)
