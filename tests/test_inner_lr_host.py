"""Per-parameter inner-loop step sizes, host side (no GPU): the ``InnerLR`` container, its place in ``MAML``, ``allow_nograd``, the
driver's flags, and the closed form the engine implements (include/mi_maml.h, mi_meta_batch_maml_lr) against fp64 autograd."""
import io

import numpy as np
import pytest
import torch

from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import InnerLR, MAML
from exploring_meta_amd.vision import maml_vision
from oracle import vision_ref as R
from helpers import model_params, task_tensors, rel_err
import inner_lr_oracle as O


@pytest.fixture(scope='module')
def model():
    torch.manual_seed(0)
    return cf.OmniglotCNN(5)


def _sizes(model):
    return [(n, p.numel()) for n, p in model.named_parameters()]


@pytest.mark.parametrize('per', ['scalar', 'tensor', 'parameter'])
@pytest.mark.parametrize('steps', [1, 3])
def test_flat_layout(model, per, steps):
    sizes = _sizes(model)
    P = sum(n for _, n in sizes)
    lr = InnerLR(model, 0.25, per=per, steps=steps)
    assert tuple(lr.values.shape) == (steps, {'scalar': 1, 'tensor': len(sizes), 'parameter': P}[per])
    assert not isinstance(lr.values, torch.nn.Parameter) and 'values' in dict(lr.named_buffers())
    flat = lr.flat()
    assert tuple(flat.shape) == (steps, P) and torch.all(flat == 0.25)
    # distinct stored values land where parameters() order puts their tensors, step by step
    with torch.no_grad():
        lr.values.copy_(torch.arange(lr.values.numel(), dtype=torch.float32).reshape(lr.values.shape))
    flat, off = lr.flat(), 0
    for i, (_, n) in enumerate(sizes):
        for s in range(steps):
            want = lr.values[s, off:off + n] if per == 'parameter' else lr.values[s, i if per == 'tensor' else 0].expand(n)
            assert torch.equal(flat[s, off:off + n], want)
        off += n


def test_frozen_prefixes_and_bad_arguments(model):
    lr = InnerLR(model, 0.5, per='tensor', frozen=('base.0.', 'linear.'))
    flat, off = lr.flat(), 0
    for name, n in _sizes(model):
        want = 0.0 if name.startswith(('base.0.', 'linear.')) else 0.5
        assert torch.all(flat[0, off:off + n] == want), name
        off += n
    extra = InnerLR(model, 0.5, per='parameter').flat(also_frozen=['base.1.conv.weight'])
    off = dict(zip([n for n, _ in _sizes(model)], np.cumsum([0] + [n for _, n in _sizes(model)][:-1])))['base.1.conv.weight']
    assert torch.all(extra[0, off:off + 64 * 64 * 9] == 0) and extra[0, off - 1] == 0.5
    with pytest.raises(ValueError, match='matches no parameter'):
        InnerLR(model, 0.5, frozen=('trunk.',))
    with pytest.raises(ValueError, match='per must be'):
        InnerLR(model, 0.5, per='layer')
    with pytest.raises(ValueError, match='steps'):
        InnerLR(model, 0.5, steps=0)


def test_per_tensor_gradient_is_the_sum_over_its_entries(model):
    lr = InnerLR(model, 0.5, per='tensor', steps=2, learnable=True, frozen=('base.0.',))
    assert isinstance(lr.values, torch.nn.Parameter)
    flat = lr.flat()
    w = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(flat.shape))).float()
    (flat * w).sum().backward()
    off = 0
    for i, (name, n) in enumerate(_sizes(model)):
        want = torch.zeros(2) if name.startswith('base.0.') else w[:, off:off + n].sum(1)
        assert torch.allclose(lr.values.grad[:, i], want, rtol=1e-5, atol=1e-5), name
        off += n
    scalar = InnerLR(model, 0.5, per='scalar', learnable=True)
    (scalar.flat() * w[:1]).sum().backward()
    assert torch.allclose(scalar.values.grad, w[:1].sum().reshape(1, 1), rtol=1e-4)


def test_maml_parameters_hold_the_step_sizes_only_when_learnable(model):
    n = len(list(model.parameters()))
    assert len(list(MAML(model, lr=0.5).parameters())) == n and MAML(model, lr=0.5).lr == 0.5
    assert MAML(model, lr=0.5).lr_flat() is None                                  # a number stays the scalar call
    fixed = MAML(model, lr=InnerLR(model, 0.5, per='tensor'))
    assert len(list(fixed.parameters())) == n and not fixed.lr_flat().requires_grad
    learn = MAML(model, lr=InnerLR(model, 0.5, per='tensor', learnable=True))
    ps = list(learn.parameters())
    assert len(ps) == n + 1 and any(p is learn.lr.values for p in ps)
    assert learn.lr_flat().requires_grad
    assert learn.clone().lr is learn.lr                                          # a clone adapts with the same step sizes
    opt = torch.optim.Adam(learn.parameters(), 0.1)                               # MetaSGD: one optimiser carries both
    assert sum(len(g['params']) for g in opt.param_groups) == n + 1


def test_state_dict_round_trip(model):
    a = InnerLR(model, 0.5, per='tensor', steps=2, learnable=True, frozen=('linear.',))
    with torch.no_grad():
        a.values.mul_(torch.linspace(0.5, 1.5, a.values.numel()).reshape(a.values.shape))
    buf = io.BytesIO()
    torch.save(a.state_dict(), buf)
    buf.seek(0)
    b = InnerLR(model, 0.1, per='tensor', steps=2, learnable=True, frozen=('linear.',))
    b.load_state_dict(torch.load(buf))
    assert torch.equal(a.flat(), b.flat())
    with pytest.raises(RuntimeError):
        InnerLR(model, 0.1, per='parameter', steps=2).load_state_dict(a.state_dict())


def test_allow_nograd_gives_frozen_parameters_step_zero():
    m = cf.OmniglotCNN(5)
    for name, p in m.named_parameters():
        p.requires_grad_(not name.startswith('base.0.'))
    assert MAML(m, lr=0.5).lr_flat() is None                                      # without allow_nograd: unchanged
    flat = MAML(m, lr=0.5, allow_nograd=True).lr_flat()
    same = InnerLR(m, 0.5, per='scalar', frozen=('base.0.',)).flat()
    assert tuple(flat.shape) == tuple(same.shape) and torch.equal(flat, same)
    both = MAML(m, lr=InnerLR(m, 0.5, per='tensor', frozen=('linear.',)), allow_nograd=True).lr_flat()
    off = 0
    for name, p in m.named_parameters():
        assert torch.all(both[0, off:off + p.numel()] == (0.0 if name.startswith(('base.0.', 'linear.')) else 0.5)), name
        off += p.numel()
    assert MAML(m, lr=0.5, allow_nograd=True).clone().lr_flat() is not None       # clones keep the flag


def test_driver_flags():
    parse = lambda argv: maml_vision.params_of(maml_vision.build_parser().parse_args(argv))
    m = cf.OmniglotCNN(5)
    p = parse([])
    assert maml_vision.inner_lr_of(m, p) == 0.5 and isinstance(maml_vision.inner_lr_of(m, p), float)      # defaults: today's scalar run
    p = parse(['--inner_lr_per', 'tensor', '--learn_inner_lr', '--per_step_lr', '--adapt_steps', '3', '--freeze', 'base.0.', 'linear.',
               '--inner_lr', '0.25'])
    lr = maml_vision.inner_lr_of(m, p)
    assert isinstance(lr, InnerLR) and (lr.per, lr.steps, lr.learnable, lr.frozen) == ('tensor', 3, True, ('base.0.', 'linear.'))
    assert float(lr.values.detach()[0, 4]) == 0.25
    lr = maml_vision.inner_lr_of(m, parse(['--freeze', 'base.0.']))
    assert isinstance(lr, InnerLR) and (lr.per, lr.steps, lr.learnable) == ('scalar', 1, False)
    assert maml_vision.inner_lr_of(m, parse(['--learn_inner_lr'])).learnable
    with pytest.raises(SystemExit):
        parse(['--inner_lr_per', 'layer'])


@pytest.mark.parametrize('K,first_order,per_step', [(1, False, False), (1, True, False), (2, False, False), (2, True, False), (2, False, True)])
def test_closed_form_equals_fp64_autograd(K, first_order, per_step):
    """What the engine computes -- lam_k = lam_{k+1} - H_k (D_k lam_{k+1}), lr_grad_k = -sum_t g_k * lam_{k+1} -- is the gradient fp64
    autograd gives through the oracle's forward with the update v - lr[name] * g.  Omniglot net, 5-way 1-shot, block 1 frozen, the other
    entries base * U(0.5, 1.5)."""
    ways, shots, tasks = 5, 1, [0, 1]
    spec = R.omniglot_spec(ways)
    theta = model_params(spec, 11)
    datas, labels = task_tensors('omni', tasks, ways, shots)
    lr = O.lr_vector(spec, 0.5 if K == 1 else 0.4, K if per_step else 1, 5)
    _, _, g, lg, _, _ = O.meta_batch(theta, spec, datas, labels, K, shots, ways, lr, first_order)
    cg, clg = O.closed_form(theta, spec, datas, labels, K, shots, ways, lr, first_order)
    assert rel_err(cg, g) <= 1e-12 and rel_err(clg, lg) <= 1e-12
    assert clg.shape == (K if per_step else 1, g.size)
    frozen = lr[0] == 0
    assert frozen.any() and np.abs(lg[0][frozen]).sum() > 0            # a step of 0 does not make its gradient 0


def test_negative_share_of_the_step_sizes_and_its_closed_form():
    """lr_vector(negative=q) flips the sign of a hashed share q of the non-frozen entries and nothing else (0: the vector as it was, bit
    for bit), and the closed form still equals fp64 autograd on such a vector (a learnt step size can cross zero): the net, tasks and
    bars of test_closed_form_equals_fp64_autograd, K = 2, one vector per step."""
    ways, shots, tasks, K = 5, 1, [0, 1], 2
    spec = R.omniglot_spec(ways)
    plain = O.lr_vector(spec, 0.4, K, 5)
    assert np.array_equal(O.lr_vector(spec, 0.4, K, 5, negative=0), plain) and (plain >= 0).all()
    lr = O.lr_vector(spec, 0.4, K, 5, negative=0.25)
    assert lr.dtype == np.float32 and np.array_equal(np.abs(lr), plain)
    live = plain != 0
    share = (lr[live] < 0).mean()
    assert 0.24 < share < 0.26, share                  # ~1.1e5 live entries per row: 0.25 +- 5 sigma is +- 0.005
    assert np.array_equal(lr, O.lr_vector(spec, 0.4, K, 5, negative=0.25))          # a pure function of its arguments
    assert not np.array_equal(lr[0] < 0, lr[1] < 0)                                 # the steps draw their signs independently
    theta = model_params(spec, 11)
    datas, labels = task_tensors('omni', tasks, ways, shots)
    _, _, g, lg, _, _ = O.meta_batch(theta, spec, datas, labels, K, shots, ways, lr, False)
    cg, clg = O.closed_form(theta, spec, datas, labels, K, shots, ways, lr, False)
    assert rel_err(cg, g) <= 1e-12 and rel_err(clg, lg) <= 1e-12
    _, _, g_plain, _, _, _ = O.meta_batch(theta, spec, datas, labels, K, shots, ways, plain, False)
    assert rel_err(g, g_plain) > 1e-3                  # the signs reach the result
