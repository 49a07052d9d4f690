"""Per-step parameter offsets in the fused MAML call, the parts that need no GPU: the closed form the engine
implements (include/mi_maml.h, mi_meta_batch_maml_offsets) against fp64 autograd, the zero-offset and final-only restatements of the
existing oracles, ``StepOffsets``, the C and Python declarations, the driver's flags and the no-GPU error."""
import os
import re

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.vision import maml_vision
from oracle import vision_ref as R
from helpers import model_params, task_tensors, rel_err
import msl_oracle as M
import step_offsets_oracle as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAYS, SHOTS, K = 5, 1, 2


def _omni(tasks=(0, 1)):
    spec = R.omniglot_spec(WAYS)
    datas, labels = task_tensors('omni', list(tasks), WAYS, SHOTS)
    return spec, model_params(spec, 11), datas, labels


@pytest.mark.parametrize('first_order', [False, True])
@pytest.mark.parametrize('vector', [False, True])
def test_closed_form_equals_fp64_autograd(first_order, vector):
    """The unchanged adjoint recursion on the shifted trajectory, with offsets_grad[k] = sum_t lam_{k+1}, is the gradient fp64 autograd
    gives with the offsets as leaves.  Omniglot net, 5-way 1-shot, tasks 0 and 1, K = 2, w = (0.3, 0.7), offsets N(0, 0.05^2) on the
    BatchNorm tensors and linear.bias; the scalar step 0.4 and the [2, P] vector.  The bar of tests/test_msl_host.py for the same kind of
    comparison."""
    w = (0.3, 0.7)
    spec, theta, datas, labels = _omni()
    lr = S.lr_vector(spec, 0.4, K, 5) if vector else 0.4
    ofs = S.offsets_array(spec, K, 31)
    ref = S.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, w, ofs, first_order)
    cg, clg, cog = S.closed_form(theta, spec, datas, labels, K, SHOTS, WAYS, lr, w, ofs, first_order)
    errs = dict(meta_grad=rel_err(cg, ref['meta_grad']), offsets_grad=rel_err(cog, ref['offsets_grad']))
    if vector:
        errs['lr_grad'] = rel_err(clg, ref['lr_grad'])
    else:
        assert clg is None and ref['lr_grad'] is None
    print('[step_offsets closed form]', first_order, vector, errs)
    assert cog.shape == ref['offsets_grad'].shape == ofs.shape
    assert all(e <= 1e-12 for e in errs.values()), errs
    # the offsets reach the result: without them the gradient is another one, and the offset gradient is not zero off the selected tensors
    plain = M.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, w, first_order)
    assert rel_err(plain['meta_grad'], ref['meta_grad']) > 1e-2 and not np.array_equal(plain['losses'][1:], ref['losses'][1:])
    assert np.array_equal(plain['losses'][0], ref['losses'][0])                    # theta_0 carries no offset
    assert np.abs(ref['offsets_grad'][:, ofs[0] == 0]).sum() > 0


@pytest.mark.parametrize('first_order', [False, True])
def test_zero_offsets_reproduce_the_msl_oracle(first_order):
    spec, theta, datas, labels = _omni()
    lr, w = S.lr_vector(spec, 0.4, K, 5), (0.3, 0.7)
    P = sum(v.numel() for v in theta.values())
    got = S.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, w, np.zeros((K, P), np.float32), first_order)
    want = M.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, w, first_order)
    for name in ('losses', 'accs', 'logits', 'meta_grad', 'lr_grad'):
        assert np.array_equal(got[name], want[name]), name
    assert got['offsets_grad'].shape == (K, P) and np.abs(got['offsets_grad']).sum() > 0


def test_final_only_weights_with_zero_offsets_are_the_step_size_oracle():
    """step_w = None (w = (0, 1)) and zero offsets restate tests/inner_lr_oracle.py; offsets_grad's last row is then the meta-gradient of
    a learner that starts at theta_K: sum_t grad L_query(theta_K)."""
    import inner_lr_oracle as O
    spec, theta, datas, labels = _omni((0,))
    lr = S.lr_vector(spec, 0.4, K, 5)
    P = sum(v.numel() for v in theta.values())
    ref = S.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, None, np.zeros((K, P), np.float32), False)
    l, _, g, lg, _, _ = O.meta_batch(theta, spec, datas, labels, K, SHOTS, WAYS, lr, False)
    assert rel_err(ref['losses'][K], l) <= 1e-14 and rel_err(ref['meta_grad'], g) <= 1e-12 and rel_err(ref['lr_grad'], lg) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- StepOffsets
def _bn_names(model):
    return [n for n, _ in model.named_parameters() if '.normalize.' in n]


def test_step_offsets_layout_and_gradient():
    model = cf.OmniglotCNN(WAYS)
    named = list(model.named_parameters())
    P = sum(p.numel() for _, p in named)
    bn = _bn_names(model)
    assert len(bn) == 8
    so = cf.StepOffsets(model, 3)
    assert isinstance(so.values, torch.nn.Parameter) and tuple(so.values.shape) == (3, 8 * 64) and float(so.values.detach().abs().sum()) == 0.0
    assert so.bn_prefixes() == tuple(bn)
    with torch.no_grad():
        so.values.copy_(torch.arange(1, 3 * 8 * 64 + 1, dtype=torch.float32).reshape(3, -1))
    flat = so.flat()
    assert tuple(flat.shape) == (3, P)
    off = col = 0
    for n, p in named:
        piece = flat[:, off:off + p.numel()]
        if n in bn:
            assert torch.equal(piece, so.values[:, col:col + p.numel()]), n
            col += p.numel()
        else:
            assert float(piece.detach().abs().sum()) == 0.0, n
        off += p.numel()
    assert col == so.values.shape[1]
    # autograd routes the gradient of the selected columns to values, and nothing else
    weight = torch.arange(3 * P, dtype=torch.float32).reshape(3, P)
    (flat * weight).sum().backward()
    want = torch.cat([weight[:, o:o + n] for o, n, name in _offsets_of(named) if name in bn], dim=1)
    assert torch.equal(so.values.grad, want)
    so.values.grad = None
    so.flat().sum().backward()
    assert torch.equal(so.values.grad, torch.ones_like(so.values))
    assert torch.equal(so.rows(), torch.cumsum(so.flat().detach(), dim=0)) and not so.rows().requires_grad
    assert 'steps=3' in repr(so)


def _offsets_of(named):
    off = 0
    for name, p in named:
        yield off, p.numel(), name
        off += p.numel()


def test_step_offsets_selections_and_bad_arguments():
    model = cf.OmniglotCNN(WAYS)
    named = list(model.named_parameters())
    P = sum(p.numel() for _, p in named)
    every = cf.StepOffsets(model, 2, 'all', init=0.25)
    assert tuple(every.values.shape) == (2, P) and torch.equal(every.flat(), torch.full((2, P), 0.25))
    assert every.bn_prefixes() == tuple(n for n, _ in named)
    some = cf.StepOffsets(model, 2, ('base.0.normalize.', 'linear.bias'), learnable=False, init=torch.tensor([[1.0], [2.0]]))
    assert not isinstance(some.values, torch.nn.Parameter) and 'values' in dict(some.named_buffers()) and not list(some.parameters())
    assert some.bn_prefixes() == ('base.0.normalize.weight', 'base.0.normalize.bias', 'linear.bias')
    assert tuple(some.values.shape) == (2, 64 + 64 + WAYS)
    flat = some.flat()
    assert float(flat[0].sum()) == 64 + 64 + WAYS and float(flat[1].sum()) == 2 * (64 + 64 + WAYS)
    assert torch.equal(some.rows()[1], flat[0] + flat[1])
    for bad in (dict(steps=0), dict(steps=1.5), dict(steps=2, tensors='batchnorm'), dict(steps=2, tensors=('nope.',)), dict(steps=2, tensors=())):
        with pytest.raises(ValueError):
            cf.StepOffsets(model, **bad)
    with pytest.raises(ValueError):
        cf.StepOffsets(torch.nn.Linear(3, 2), 2)                                   # 'bn' without a BatchNorm tensor
    with pytest.raises(ValueError):
        cf.StepOffsets(torch.nn.ReLU(), 2, 'all')                                  # no parameters


def test_maml_carries_the_offsets():
    model = cf.OmniglotCNN(WAYS)
    plain = cf.MAML(model, lr=0.4)
    assert plain.offsets is None and plain.offsets_flat() is None and plain.clone().offsets_flat() is None
    n_model = len(list(model.parameters()))
    assert len(list(plain.parameters())) == n_model
    so = cf.StepOffsets(model, 2)
    maml = cf.MAML(model, lr=0.4, offsets=so)
    assert len(list(maml.parameters())) == n_model + 1 and any(q is so.values for q in maml.parameters())
    assert maml.clone().offsets is so and torch.equal(maml.clone().offsets_flat(), so.flat())
    frozen = cf.MAML(model, lr=0.4, offsets=cf.StepOffsets(model, 2, learnable=False))
    assert len(list(frozen.parameters())) == n_model
    with pytest.raises(TypeError):
        cf.MAML(model, lr=0.4, offsets=torch.zeros(2, 3))


# ---------------------------------------------------------------------------------------------------------------- declarations
def test_symbols_are_declared_and_bound():
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    names = ('mi_meta_batch_maml_offsets', 'mi_workspace_bytes_offsets')
    for name in names:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert name in _lib._SIGS and name in _lib.EXPORTS
    for name in names:                                                             # one argument type per parameter of the declaration
        decl = re.search(r'\bint\s+' + name + r'\s*\(([^;]*)\)\s*;', header).group(1)
        assert len(decl.split(',')) == len(_lib._SIGS[name][1]), name
    assert 'Antoniou' in header[header.index('PER-STEP PARAMETER OFFSETS'):header.index('mi_workspace_bytes_offsets')]
    assert callable(cf.StepOffsets) and callable(cf.meta_batch_adapt) and callable(cf.meta_batch_adapt_steps)


def test_driver_flags():
    parse = lambda argv: maml_vision.params_of(maml_vision.build_parser().parse_args(argv))
    p = parse([])
    assert p['per_step_bn'] is False and p['per_step_bn_adapt_bn'] is False and p['first_order_iterations'] == 0
    assert p['cosine_outer_lr'] is False and p['min_outer_lr'] == 0.0
    model = cf.OmniglotCNN(WAYS)
    assert maml_vision.inner_lr_of(model, p) == p['inner_lr'] and maml_vision.step_offsets_of(model, p) is None   # defaults: today's objects
    bn = tuple(_bn_names(model))
    p = parse(['--per_step_bn', '--adapt_steps', '3', '--first_order_iterations', '4', '--cosine_outer_lr', '--min_outer_lr', '1e-5'])
    assert p['per_step_bn'] is True and p['first_order_iterations'] == 4 and p['cosine_outer_lr'] is True and p['min_outer_lr'] == 1e-5
    so, lr = maml_vision.step_offsets_of(model, p), maml_vision.inner_lr_of(model, p)
    assert isinstance(so, cf.StepOffsets) and (so.steps, so.learnable, so.bn_prefixes()) == (3, True, bn)
    assert isinstance(lr, cf.InnerLR) and (lr.per, lr.steps, lr.learnable, lr.frozen) == ('scalar', 1, False, bn)
    flat = lr.flat()
    assert float(flat.max()) == p['inner_lr'] and int((flat == 0).sum()) == 8 * 64
    p = parse(['--per_step_bn', '--adapt_steps', '2', '--freeze', 'base.0.', '--inner_lr_per', 'tensor', '--learn_inner_lr'])
    lr = maml_vision.inner_lr_of(model, p)
    assert lr.frozen == ('base.0.',) + tuple(n for n in bn if not n.startswith('base.0.')) and lr.per == 'tensor' and lr.learnable
    p = parse(['--per_step_bn', '--per_step_bn_adapt_bn', '--adapt_steps', '2'])
    assert maml_vision.inner_lr_of(model, p) == p['inner_lr'] and maml_vision.step_offsets_of(model, p).steps == 2
    with pytest.raises(ValueError):
        maml_vision.step_offsets_of(model, parse(['--per_step_bn', '--adapt_steps', '0']))


@pytest.mark.skipif(torch.cuda.is_available(), reason='the no-GPU error shows where there is no GPU')
def test_offsets_call_needs_a_gpu():
    model = cf.OmniglotCNN(WAYS)
    data, labels = torch.zeros(1, 10, 1, 28, 28), torch.zeros(1, 10, dtype=torch.int64)
    maml = cf.MAML(model, lr=0.4, offsets=cf.StepOffsets(model, 2))
    with pytest.raises(RuntimeError, match='only on the GPU'):                        # what meta_batch_adapt raises there (no CPU fallback)
        cf.meta_batch_adapt(maml.clone(), data, labels, 2, 1, 5)
    with pytest.raises(RuntimeError, match='only on the GPU'):
        cf.meta_batch_adapt_steps(maml.clone(), data, labels, 2, 1, 5, step_weights=[0.3, 0.7])
