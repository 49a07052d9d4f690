"""CPU tests of the vector-step / multi-step-loss ANIL calls: the closed form the engine implements against fp64
autograd (tests/anil_steps_oracle.py), the oracle against the reference restatement it extends, the margin property the GPU test relies
on, the step-size layout of a Linear head, the driver's flags, the C symbols and the no-GPU refusals."""
import re
import os

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from oracle import vision_ref as R
import anil_steps_oracle as A

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lr(kind, fc, ways, K):
    if kind == 'scalar':
        return 0.4
    if kind == 'per_step':
        return A.lr_vector(fc, ways, 0.4, K, 5)
    if kind == 'frozen_bias':
        return A.lr_vector(fc, ways, 0.4, 1, 5, frozen=('bias',))
    raise KeyError(kind)


@pytest.mark.parametrize('fo', [False, True])
@pytest.mark.parametrize('kind', ['scalar', 'per_step', 'frozen_bias'])
@pytest.mark.parametrize('K', [1, 3])
def test_closed_form_is_autograd(K, kind, fo):
    """Trunk gradient, head gradient and lr_grad of the closed form = fp64 autograd of sum_j w_j L_q(theta_j) to 1e-12."""
    base, tf, th, fc, ways, shots = A.fixtures('omni')
    datas, labels = A.tasks('omni', [0, 1])
    w = {1: (0.7,), 3: (0.2, 0.3, 0.5)}[K]
    lr = _lr(kind, fc, ways, K)
    want = A.meta_batch(tf, th, base, fc, datas, labels, K, shots, ways, lr, w, fo)
    gf, gh, lg = A.closed_form(tf, th, base, fc, datas, labels, K, shots, ways, lr, w, fo)
    assert A.rel_err(gf, want['grad_feat']) < 1e-12 and A.rel_err(gh, want['grad_head']) < 1e-12
    assert np.abs(want['grad_feat']).sum() > 0 and np.abs(want['grad_head']).sum() > 0
    if kind == 'scalar':
        assert lg is None and want['lr_grad'] is None
    else:
        assert lg.shape == want['lr_grad'].shape == (K if kind == 'per_step' else 1, A.head_count(fc, ways))
        assert A.rel_err(lg, want['lr_grad']) < 1e-12 and np.abs(lg).sum() > 0
        if kind == 'frozen_bias':
            assert np.abs(lg[:, ways * fc:]).sum() > 0       # a step of 0 still has a gradient


@pytest.mark.parametrize('fo', [False, True])
def test_final_only_uniform_vector_is_the_reference_restatement(fo):
    """w = (0, 1) with a uniform vector: losses, accuracies and gradients of R.anil_meta_batch."""
    K, lr = 2, 0.4
    base, tf, th, fc, ways, shots = A.fixtures('omni')
    datas, labels = A.tasks('omni', [0, 1])
    l64, a64, gf, gh = R.anil_meta_batch(tf, th, base, fc, datas, labels, K, shots, ways, lr, first_order=fo)
    got = A.meta_batch(tf, th, base, fc, datas, labels, K, shots, ways, np.full((1, A.head_count(fc, ways)), lr), (0.0, 1.0), fo)
    assert np.allclose(got['losses'][K], l64.numpy(), rtol=1e-13) and np.array_equal(got['accs'][K], a64.numpy().astype(np.float64))
    assert A.rel_err(got['grad_feat'], R.flatten_params(gf).numpy()) < 1e-12
    assert A.rel_err(got['grad_head'], R.flatten_params(gh).numpy()) < 1e-12
    for j in range(K):      # ... and row j is the reference adapted for j steps
        lj, aj, _, _ = R.anil_meta_batch(tf, th, base, fc, datas, labels, j, shots, ways, lr, first_order=fo, backward=False)
        assert np.allclose(got['losses'][j], lj.numpy(), rtol=1e-13) and np.array_equal(got['accs'][j], aj.numpy().astype(np.float64))


@pytest.mark.parametrize('case', list(A.ORACLE_CASES))
def test_oracle_margins_of_the_gpu_cases(case):
    """The GPU test compares per-step accuracy on the rows whose fp64 top-2 margin is clear and may leave out at most one row in ten of
    any (step, task): the fp64 oracle alone meets that on every case the GPU test runs (its task ids, step sizes and K)."""
    shape, ids, K = A.ORACLE_CASES[case][:3]
    ways, shots = A.SHAPES[shape][4:]
    clear = A.clear_rows(A.case_oracle(case)['logits'])
    assert clear.shape == (K + 1, len(ids), ways * shots)
    assert np.all((~clear).sum(axis=-1) * 10 <= ways * shots), (~clear).sum(axis=-1)


def test_lr_flat_layout_of_a_linear_head():
    """MAML(Linear, lr=InnerLR).lr_flat() is [steps, Ph] in the order weight (row-major [ways, fc]), bias: the order of lr_vec."""
    ways, fc, K = 3, 8, 2
    head = torch.nn.Linear(fc, ways)
    assert cf.MAML(head, lr=0.4).lr_flat() is None
    init = torch.tensor([[0.1, 0.2], [0.3, 0.4]])
    il = cf.InnerLR(head, init, per='tensor', steps=K, learnable=True)
    flat = cf.MAML(head, lr=il).lr_flat()
    assert tuple(flat.shape) == (K, ways * fc + ways) and flat.requires_grad
    assert torch.all(flat[0, :ways * fc] == 0.1) and torch.all(flat[0, ways * fc:] == 0.2) and torch.all(flat[1, ways * fc:] == 0.4)
    (flat * torch.arange(flat.numel()).reshape(flat.shape)).sum().backward()
    assert il.values.grad is not None and float(il.values.grad.abs().sum()) > 0
    head.bias.requires_grad_(False)
    frozen = cf.MAML(head, lr=0.4, allow_nograd=True).lr_flat()
    assert tuple(frozen.shape) == (1, ways * fc + ways) and torch.all(frozen[0, :ways * fc] == 0.4) and torch.all(frozen[0, ways * fc:] == 0)


def test_driver_flags():
    from exploring_meta_amd.vision import anil_vision
    p = anil_vision.parse_args([])
    assert p.inner_lr_per == 'scalar' and p.msl_iterations == 0 and not p.learn_inner_lr and not p.per_step_lr and not p.freeze and not p.multi_step_loss
    p = anil_vision.parse_args(['--inner_lr_per', 'tensor', '--learn_inner_lr', '--per_step_lr', '--freeze', 'bias', '--multi_step_loss',
                                '--msl_iterations', '7'])
    assert p.inner_lr_per == 'tensor' and p.learn_inner_lr and p.per_step_lr and p.freeze == ['bias'] and p.multi_step_loss
    assert p.msl_iterations == 7


def test_symbols_declared_and_bound():
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    for name in ('mi_anil_workspace_bytes_steps', 'mi_meta_batch_anil_lr', 'mi_meta_batch_anil_steps'):
        assert re.search(r'\bint ' + name + r'\(', header), name
        assert name in _lib.EXPORTS
    nargs = lambda name: len(_lib._SIGS[name][1])
    decl = lambda name: re.search(r'\bint ' + name + r'\(([^;]*)\);', header).group(1).count(',') + 1
    for name in ('mi_anil_workspace_bytes_steps', 'mi_meta_batch_anil_lr', 'mi_meta_batch_anil_steps'):
        assert nargs(name) == decl(name), name


@pytest.mark.skipif(torch.cuda.is_available(), reason='checks the refusal on a machine without a GPU')
def test_calls_raise_without_a_gpu():
    from exploring_meta_amd.engine import MetaEngine, ModelSpec
    with pytest.raises(_lib.MiError):
        MetaEngine(ModelSpec.anil(5, hidden=32, channels=1, max_pool=False, in_hw=28))
    head = cf.MAML(torch.nn.Linear(128, 5), lr=cf.InnerLR(torch.nn.Linear(128, 5), 0.4, per='tensor'))
    trunk = torch.nn.Sequential(cf.ConvBase(output_size=32, hidden=32, channels=1, max_pool=False))
    data, labels = torch.zeros(1, 10, 1, 28, 28), torch.zeros(1, 10, dtype=torch.int64)
    with pytest.raises(Exception):
        cf.meta_batch_adapt_anil(head, trunk, data, labels, 1, 1, 5)
    with pytest.raises(Exception):
        cf.meta_batch_adapt_anil_steps(head, trunk, data, labels, 1, 1, 5)
