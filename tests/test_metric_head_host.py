"""CPU tests of the metric heads: the closed form the kernel implements against fp64 autograd of the definitions
(tests/metric_head_oracle.py), the margin property the GPU test relies on, the drivers' flags, the C symbols, and what the Python
surface refuses without a GPU."""
import functools
import re

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
import metric_head_oracle as M
from closed_form_utils import symbols_declared_and_bound

SYMBOLS = ('mi_metric_head_scratch_bytes', 'mi_metric_head', 'mi_metric_workspace_bytes', 'mi_meta_batch_metric')


@pytest.mark.parametrize('metric', [M.PROTO, M.COSINE])
@pytest.mark.parametrize('feat,ways,ns,nq,T', [(33, 3, 6, 4, 2), (16, 5, 5, 7, 1), (128, 1, 3, 3, 1)])
def test_closed_form_is_autograd(feat, ways, ns, nq, T, metric):
    """Loss, logits, dfs and dfq of the closed form = fp64 autograd of the definitions to 1e-10, with unbalanced classes (counts 1, 2, 3)
    and ns != nq."""
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, ns, nq, T)
    if (ways, ns) == (3, 6):
        assert sorted(np.bincount(ys[0], minlength=ways)) == [1, 2, 3]
    scale = 0.25 if metric == M.PROTO else 3.0
    want = M.head(fs, fq, ys, yq, ways, metric, scale)
    got = M.closed_form(fs, fq, ys, yq, ways, metric, scale)
    assert np.allclose(got[1], want[1], rtol=0, atol=1e-6)                 # (the oracle's accuracy is vision_ref's fp32 ratio)
    for name, a, b in zip(('loss', 'logits', 'dfs', 'dfq'), got[:1] + got[2:], want[:1] + want[2:]):
        assert a.shape == b.shape and (M.rel_err(a, b) < 1e-10 or (np.abs(b).max() == 0 and np.abs(a).max() < 1e-300)), (name, M.rel_err(a, b))
    if ways > 1:
        assert np.abs(want[3]).sum() > 0 and np.abs(want[4]).sum() > 0


def test_closed_form_clamp_branch_is_autograd():
    """cosine with a zero support row and a zero query row: the 1e-8 clamp, dx = dxh / 1e-8 -- finite, and what autograd gives."""
    fs, fq, ys, yq = M.kernel_inputs(16, 3, 6, 4, 1)
    fs[0, 1] = 0.0
    fq[0, 2] = 0.0
    want = M.head(fs, fq, ys, yq, 3, M.COSINE, 2.0)
    got = M.closed_form(fs, fq, ys, yq, 3, M.COSINE, 2.0)
    for a, b in zip(got[:1] + got[2:], want[:1] + want[2:]):
        assert np.isfinite(a).all() and M.rel_err(a, b) < 1e-10
    assert np.abs(want[3][0, 1]).max() > 1e6 and np.abs(want[4][0, 2]).max() > 1e6       # dxh / 1e-8


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    return M.case_oracle(shape)


@pytest.mark.parametrize('metric', [M.PROTO, M.COSINE])
@pytest.mark.parametrize('shape', list(M.FUSED_CASES))
def test_oracle_margins_of_the_gpu_cases(shape, metric):
    """The GPU test compares accuracy on the rows whose fp64 top-2 margin is clear and may leave out at most one row in ten of a task: the
    fp64 oracle alone meets that on every fused-call case.  The cases also test something: losses inside [0.36, 1.41], no accuracy of 0."""
    ids = M.FUSED_CASES[shape][0]
    ways, shots = M.SHAPES[shape][4:]
    o = _oracle(shape)[metric]
    clear = M.clear_rows(o['logits'][None])[0]
    print(f'[margin] {shape} {metric}: losses {o["losses"]}, accs {o["accs"]}, unclear rows per task {(~clear).sum(axis=-1)}')
    assert clear.shape == (len(ids), ways * shots)
    assert np.all((~clear).sum(axis=-1) * 10 <= ways * shots), (~clear).sum(axis=-1)
    assert np.all(o['losses'] > 0.36) and np.all(o['losses'] < 1.41) and np.all(o['accs'] > 0), (o['losses'], o['accs'])
    assert np.abs(o['grad_feat']).sum() > 0


def test_symbols_declared_and_bound():
    header = symbols_declared_and_bound(SYMBOLS)
    assert re.search(r'#define MI_METRIC_PROTO 0\b', header) and re.search(r'#define MI_METRIC_COSINE 1\b', header)
    from exploring_meta_amd.engine import METRICS
    assert METRICS == {'proto': 0, 'cosine': 1}


def test_driver_flags():
    from exploring_meta_amd.vision import anil_vision, maml_vision, protonet_vision
    p = protonet_vision.build_parser().parse_args([])
    assert p.metric == 'proto' and p.scale == 1.0 and p.dataset == 'min' and p.save_dir == ''
    p = protonet_vision.build_parser().parse_args(['--dataset', 'omni', '--metric', 'cosine', '--scale', '4', '--save_dir', 'x'])
    assert p.metric == 'cosine' and p.scale == 4.0 and p.dataset == 'omni' and p.save_dir == 'x'
    with pytest.raises(SystemExit):
        protonet_vision.build_parser().parse_args(['--metric', 'euclid'])
    for mod in (anil_vision, maml_vision):
        assert not mod.build_parser().parse_args([]).nil_test and mod.build_parser().parse_args(['--nil_test']).nil_test
        assert mod.params_of(mod.build_parser().parse_args([]))['nil_test'] is False


def test_the_surface_refuses_without_a_gpu():
    """An unknown metric, scale <= 0 and an OmniglotCNN are refused before anything touches a device."""
    trunk = torch.nn.Sequential(cf.ConvBase(output_size=32, hidden=32, channels=1, max_pool=False))
    data, labels = torch.zeros(1, 10, 1, 28, 28), torch.zeros(1, 10, dtype=torch.int64)

    class Tasks:
        def sample(self):
            raise AssertionError('refused before a task is drawn')
    p = dict(meta_batch_size=2, shots=1, ways=5)
    with pytest.raises(_lib.MiError, match='unknown metric'):
        cf.meta_batch_adapt_metric(trunk, data, labels, 1, 5, metric='euclid')
    with pytest.raises(_lib.MiError, match='unknown metric'):
        cf.evaluate_nil(p, Tasks(), trunk, 'cpu', metric='euclid')
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(_lib.MiError, match='scale must be positive'):
            cf.meta_batch_adapt_metric(trunk, data, labels, 1, 5, scale=bad)
        with pytest.raises(_lib.MiError, match='scale must be positive'):
            cf.fast_adapt_metric((data[0], labels[0]), trunk, 1, 5, 'cpu', scale=bad)
        with pytest.raises(_lib.MiError, match='scale must be positive'):
            cf.evaluate_nil(p, Tasks(), trunk, 'cpu', scale=bad)
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.evaluate_nil(p, Tasks(), cf.OmniglotCNN(5), 'cpu')
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.meta_batch_adapt_metric(cf.OmniglotCNN(5), data, labels, 1, 5)
    from exploring_meta_amd.engine import MetaEngine
    assert callable(MetaEngine.meta_batch_metric) and callable(MetaEngine.metric_head)


@pytest.mark.parametrize('metric', (M.PROTO, M.COSINE))
def test_edge_cases_take_the_paths_they_are_there_for(metric):
    """Settled on the fp64 reference alone: every edge case is inside the header's LDS inequality (the 64-way one at 37848 of 40960
    floats), keeps the contract N_w >= 1, has a loss above 1e-3 and gradients that are not zero; the 64-way query labels reach lanes 32 to
    63; (8, 9) classes are one full chunk of 8 and one class into the second; 515 is odd and above one trip of the 512 threads."""
    assert M.lds_floats(64, 70, 515, 64) == 37848
    assert [c[1] for c in M.EDGE_CASES[1:3]] == [8, 9] and M.EDGE_CASES[0][0] == 515 and 515 % 2 == 1 and 515 > 512 and M.EDGE_CASES[3][3] > 64
    for feat, ways, ns, nq, T in M.EDGE_CASES:
        assert M.lds_floats(ns, nq, feat, ways) <= 40960
        fs, fq, ys, yq = M.kernel_inputs(feat, ways, ns, nq, T)
        assert all(np.bincount(y, minlength=ways).min() >= 1 for y in ys)
        loss, _, _, dfs, dfq = M.head(fs, fq, ys, yq, ways, metric, (1.0 / feat) if metric == M.PROTO else 4.0)
        assert np.all(loss > 1e-3) and np.abs(dfs).sum() > 0 and np.abs(dfq).sum() > 0
    assert set(M.kernel_inputs(515, 64, 64, 70, 1)[3][0].tolist()) == set(range(64))


def test_kernel_inputs_labels():
    """ns < ways takes ABSENT's labels, explicit labels win, everything else is as it was."""
    assert M.kernel_inputs(8, 5, 3, 4, 2)[2].tolist() == [[0, 2, 4]] * 2 and M.kernel_inputs(8, 2, 1, 1, 1)[2].tolist() == [[1]]
    assert M.kernel_inputs(8, 5, 3, 4, 1, ys=(4, 0, 2))[2].tolist() == [[4, 0, 2]]
    assert M.kernel_inputs(8, 3, 6, 4, 1)[2].tolist() == [[0, 1, 1, 2, 2, 2]] and M.kernel_inputs(8, 5, 10, 4, 1)[2].tolist() == [[0, 0, 1, 1, 2, 2, 3, 3, 4, 4]]
    with pytest.raises(AssertionError):
        M.kernel_inputs(8, 5, 3, 4, 1, ys=(0, 2, 5))
