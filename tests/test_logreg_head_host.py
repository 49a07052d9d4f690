"""CPU tests of the logistic-regression head: the kernel's formulas and solver restated in NumPy
(logreg_head_oracle.closed_form) against fp64 autograd of the definition (``head``), the optimum against the loop whose limit it is, the
solver's counts against the caps of the header, the conditions the GPU test puts on its cases, the bar 2^-23 + 2 e_dp + 2 e_ref on an fp64
model of the kernel and on two mutants that must break it, the header's LDS formula and domain, the drivers' flags, the C symbols, and
what the Python surface refuses without a GPU."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
import logreg_head_oracle as LH
from closed_form_utils import symbols_declared_and_bound

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mi_logreg_head_scratch_bytes', 'mi_logreg_head', 'mi_logreg_workspace_bytes', 'mi_meta_batch_logreg')
NAMES = ('loss', 'acc', 'logits', 'dfs', 'dfq', 'dhyper')

# every case the GPU test sends through its bar: the kernel cases, the edge cases, and test_domain_limits' feat = MI_RIDGE_MAX_FEAT
BAR_CASES = [c + h for c in LH.ALL_CASES for h in LH.HYPERS] + [(LH.MAX_FEAT, 5, 5, 5, 1, 1.0, 1.0)]
BAR_IDS = ['-'.join(f'{v:g}' for v in c) for c in BAR_CASES]


@functools.lru_cache(maxsize=None)
def _refs(case):
    """(inputs, head, closed_form without its counts, the counts) of a BAR_CASES entry, shared by the tests below (never modified)."""
    feat, ways, ns, nq, T, lam, alpha = case
    inputs = LH.kernel_inputs(feat, ways, ns, nq, T)
    *cf_, info = LH.closed_form(*inputs, ways, lam, alpha)
    return inputs, LH.head(*inputs, ways, lam, alpha), tuple(cf_), info


def _model(case, **kw):
    """The kernel's arithmetic as the header states it, in NumPy: fp64 everywhere, no fp32 intermediate, every output rounded to fp32."""
    inputs = _refs(case)[0]
    return LH.closed_form(*inputs, case[1], case[5], case[6], round_out=True, **kw)[:-1]


def _bar(case, got):
    _, o64, ocf, _ = _refs(case)
    return LH.bar_errors(got, o64, ocf)


@pytest.mark.parametrize('case', BAR_CASES, ids=BAR_IDS)
def test_closed_form_is_the_definition(case):
    """Loss, logits, dfs, dfq, dlam and dalpha of the kernel's formulas and solver = fp64 autograd through Newton steps at the optimum found
    with a dense solve, to 1e-9; the accuracy is equal."""
    _, want, got, info = _refs(case)
    assert info['flagged'] == 0 and info['residual'] <= LH.ACCEPT
    assert np.allclose(got[1], want[1], rtol=0, atol=1e-6)                 # (the oracle's accuracy is vision_ref's fp32 ratio)
    for name, a, b in zip(NAMES, got, want):
        if name == 'acc':
            continue
        assert a.shape == b.shape and (LH.rel(a, b) < 1e-9 or (np.abs(b).max() == 0 and np.abs(a).max() == 0)), (name, LH.rel(a, b))


def test_the_optimum_is_the_limit_of_gradient_descent():
    """20000 steps of plain gradient descent on sum_i CE(W fs_i, ys_i) + lam/2 |W|^2 from W = 0 (step 1 / L, L = lam + lambda_max(G) / 2, a
    bound on the Hessian) end at W* = A^T Fs of the dual solution to 1e-6: the head is what ANIL's inner loop tends to under its own loss."""
    feat, ways, ns, nq, lam = 33, 5, 5, 5, 1.0
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, ns, nq, 1)
    s = fs[0].astype(np.float64)
    y = np.eye(ways)[ys[0]]
    g = torch.from_numpy(s @ s.T)
    a = LH.solve_dual(g, torch.from_numpy(ys[0]).long(), ways, lam).numpy()
    w_star = a.T @ s
    step = 1.0 / (lam + 0.5 * float(np.linalg.eigvalsh(s @ s.T)[-1]))
    w = np.zeros((ways, feat))
    for _ in range(20000):
        z = s @ w.T
        p = np.exp(z - z.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        w -= step * ((p - y).T @ s + lam * w)
    assert LH.rel(w, w_star) < 1e-6, LH.rel(w, w_star)
    assert LH.rel(w, np.zeros_like(w) + w_star.mean()) > 1e-2              # (and W* is not trivial)


def test_every_case_stays_within_half_of_each_cap():
    """The Newton, CG and halving counts of the kernel's solver on every kernel, edge, limit and fused case are at most half of
    MI_LOGREG_NEWTON_CAP, MI_LOGREG_CG_CAP and MI_LOGREG_HALVE_CAP as include/mi_maml.h defines them."""
    caps = LH.caps()
    assert caps == dict(newton=32, cg=256, halve=8)
    worst = dict(newton=0, cg=0, halve=0)
    for case in BAR_CASES:
        info = _refs(case)[3]
        for k in worst:
            worst[k] = max(worst[k], info[k])
    for shape in LH.FUSED_CASES:
        info = _fused_features(shape)[1]
        for k in worst:
            worst[k] = max(worst[k], info[k])
    print(f'[counts] the most over every case: {worst}; caps {caps}')
    for k in worst:
        assert 2 * worst[k] <= caps[k], (k, worst[k], caps[k])
    assert worst['newton'] >= 8 and worst['cg'] >= 40 and worst['halve'] >= 1        # (the cases do exercise the loops and a halving)


@pytest.mark.parametrize('case', BAR_CASES, ids=BAR_IDS)
def test_cases_meet_the_conditions_the_gpu_test_rests_on(case):
    """Settled on the fp64 reference alone.  ways > 1: every task's loss inside [0.05, 5] and no gradient zero, so a relative bar means
    something; every row's top-2 logit margin is at least 10 x what the bar lets two returned logits move against each other (twice the
    row's bar times the row's norm), so `argmax equal on every row` cannot turn on a rounding.  One class: zero Newton steps, all zero."""
    _, o64, ocf, info = _refs(case)
    ways = case[1]
    if ways == 1:
        assert np.all(o64[0] == 0) and np.all(o64[5] == 0) and info['newton'] == 0 and info['cg'] == 0
        return
    assert np.all(o64[0] >= 0.05) and np.all(o64[0] <= 5.0), o64[0]
    assert np.abs(o64[3]).sum() > 0 and np.abs(o64[4]).sum() > 0 and np.all(o64[5] != 0), o64[5]
    bar = LH.bar_errors(o64, o64, ocf)['logits_rows'][1]
    z = o64[2].reshape(-1, ways)
    top2 = np.sort(z, axis=-1)[:, -2:]
    margin, moves = top2[:, 1] - top2[:, 0], 2 * bar * np.linalg.norm(z, axis=-1)
    print(f'[case] {case}: loss {o64[0]}, smallest margin {margin.min():.3e}, largest move {moves.max():.3e}')
    assert np.all(margin > 10 * moves), (margin.min(), moves.max())


@pytest.mark.parametrize('case', BAR_CASES, ids=BAR_IDS)
def test_the_kernels_model_stays_inside_the_bar(case):
    """fp64 arithmetic with fp32 stores meets 2^-23 + 2 e_ref on every quantity and on every row of logits, dfs and dfq."""
    res = _bar(case, _model(case))
    print(f'[bar, model] {case}: ' + ', '.join(f'{n} {np.max(e):.2e} ({np.max(e / b):.2f} of its bar)' for n, (e, b) in res.items()))
    for n, (err, bar) in res.items():
        assert np.all(err <= bar), (n, np.max(err / bar))


GRAM_MUTANT = [c for c in BAR_CASES if c[2] >= 20 or c[0] == LH.MAX_FEAT]
SOLVER_MUTANT = [c for c in BAR_CASES if c[:5] in ((1600, 5, 25, 25, 2), (128, 3, 6, 4, 1), (515, 5, 3, 75, 2), (LH.MAX_FEAT, 5, 5, 5, 1))]


@pytest.mark.parametrize('case', GRAM_MUTANT, ids=['-'.join(f'{v:g}' for v in c) for c in GRAM_MUTANT])
def test_an_fp32_gram_matrix_breaks_the_bar(case):
    """The bar has teeth: the same model with Fs Fs^T accumulated in fp32 is rejected on the logits, over all and on some row, in every case
    with 20 or more support rows and at feat = 65536; with 25 or more rows, or 36 ways, on dfs and dfq as well."""
    res = _bar(case, _model(case, gram_dtype=np.float32))
    print(f'[bar, fp32 Gram] {case}: ' + ', '.join(f'{n} {np.max(e / b):.2f}' for n, (e, b) in res.items()))
    broken = ('logits', 'logits_rows') + (('dfs', 'dfq') if case[2] >= 25 or case[0] == LH.MAX_FEAT else ())
    for n in broken:
        assert np.max(res[n][0] / res[n][1]) > 1, (n, np.max(res[n][0] / res[n][1]))


@pytest.mark.parametrize('case', SOLVER_MUTANT, ids=['-'.join(f'{v:g}' for v in c) for c in SOLVER_MUTANT])
def test_a_solver_satisfied_with_1e_5_breaks_the_bar(case):
    """The same model with the residual it accepts loosened from 1e-10 to 1e-5 (and stopping there) is rejected on every quantity."""
    *got, info = LH.closed_form(*_refs(case)[0], case[1], case[5], case[6], round_out=True, stop=1e-5, accept=1e-5)
    assert info['flagged'] == 0 and 1e-10 < info['residual'] <= 1e-5
    res = _bar(case, got)
    print(f'[bar, 1e-5 solver] {case}: ' + ', '.join(f'{n} {np.max(e / b):.2f}' for n, (e, b) in res.items()))
    for n in LH.QUANTITIES:
        assert np.max(res[n][0] / res[n][1]) > 1, (n, np.max(res[n][0] / res[n][1]))


def test_flagged_tasks_of_the_model():
    """A NaN in task 1's support features: the model flags that task alone (every output NaN) and leaves the others finite; the caps
    themselves flag a task that cannot converge within them (a cap of one Newton step)."""
    fs, fq, ys, yq = LH.flag_inputs()
    *got, info = LH.closed_form(fs, fq, ys, yq, 2, 1.0, 1.0)
    assert info['flagged'] == 1
    for g in got:
        assert np.all(np.isnan(g[1])) and np.isfinite(g[::2]).all()
    *got, info = LH.closed_form(*LH.kernel_inputs(33, 5, 5, 5, 1), 5, 1.0, 1.0, cap=dict(newton=1, cg=256, halve=8))
    assert info['flagged'] == 1 and all(np.all(np.isnan(g)) for g in got)


# ---------------------------------------------------------------------------------------------------------------- the fused-call cases
@functools.lru_cache(maxsize=None)
def _oracle(shape):
    return LH.case_oracle(shape)


@functools.lru_cache(maxsize=None)
def _fused_features(shape):
    """(the oracle's dict, the solver's counts on the case's fp64 features rounded to fp32)."""
    from collections import OrderedDict
    from oracle import vision_ref as R
    ids, lam, alpha = LH.FUSED_CASES[shape]
    base, tf, _, fc, ways, shots = LH.fixtures(shape, torch.float64)
    datas, labels = LH.tasks(shape, list(ids), torch.float64)
    fl = OrderedDict((k, v.detach().double()) for k, v in tf.items())
    parts = []
    with torch.no_grad():
        for d, l in zip(datas, labels):
            fs, ys, fq, yq = R.prepare_batch(d.double(), l, shots, ways, lambda x: R.conv_base(x, fl, base, prefix='0.').view(-1, fc))
            parts.append([t.numpy() for t in (fs, fq, ys, yq)])
    fs, fq, ys, yq = (np.stack(p) for p in zip(*parts))
    *_, info = LH.closed_form(fs.astype(np.float32), fq.astype(np.float32), ys, yq, ways, lam, alpha)
    return _oracle(shape), info


@pytest.mark.parametrize('shape', list(LH.FUSED_CASES))
def test_oracle_conditions_of_the_fused_cases(shape):
    """What the GPU test needs of its fused-call inputs, met by the fp64 reference alone at the (lam, alpha) fixed here: every task's loss
    inside [0.05, 3] (neither saturated nor untrained), no query row under the accuracy margin, gradients that are not zero."""
    assert LH.FUSED_CASES == {'omni': ((0, 1, 2, 3), 1.0, 1.0), 'omni3w2s': ((0, 1, 2), 1.0, 1.0), 'min': ((0, 1, 2), 1.0, 0.25)}
    ids = LH.FUSED_CASES[shape][0]
    ways, shots = LH.SHAPES[shape][4:]
    o, info = _fused_features(shape)
    clear = LH.clear_rows(o['logits'][None])[0]
    print(f'[logreg cases] {shape} (lam, alpha) = {LH.FUSED_CASES[shape][1:]}: losses {o["losses"]}, accs {o["accs"]}, '
          f'unclear rows per task {(~clear).sum(axis=-1)}, dhyper {o["dhyper"].tolist()}, counts {info}')
    assert clear.shape == (len(ids), ways * shots) and clear.all()
    assert np.all(o['losses'] >= 0.05) and np.all(o['losses'] <= 3.0), o['losses']
    assert np.abs(o['grad_feat']).sum() > 0 and np.all(o['dhyper'] != 0)
    assert info['flagged'] == 0 and LH.lds_bytes(ways * shots, ways * shots, ways) <= 163840


# ---------------------------------------------------------------------------------------------------------------- cases, domain, surface
def test_kernel_cases_and_the_domain():
    """The kernel-entry cases are metric_head_oracle's; the edge cases are the ones the header's paths need; every one is inside the LDS
    inequality of the header, which holds ns = nq = 25 at 5 ways and ns = nq = 20 at 20 ways; the 36-way case needs the dynamic-LDS attribute
    and its labels reach lanes 32 to 35."""
    assert LH.KERNEL_CASES == list(LH.M.KERNEL_CASES)
    assert LH.EDGE_CASES == [(515, 36, 36, 40, 1), (515, 5, 3, 75, 2), (4, 2, 1, 1, 1), (5, 1, 1, 3, 1), (1, 5, 5, 5, 1)]
    assert LH.HYPERS == [(1.0, 1.0), (50.0, 1.0)]
    for feat, ways, ns, nq, T in LH.ALL_CASES:
        assert LH.lds_bytes(ns, nq, ways) <= 163840 and feat <= LH.MAX_FEAT and ways <= 64
    assert LH.lds_bytes(25, 25, 5) == 22256 and LH.lds_bytes(20, 20, 20) == 42656 and LH.lds_bytes(5, 5, 5) == 3056
    assert 64 * 1024 < LH.lds_bytes(36, 40, 36) == 138880 <= 163840 < LH.lds_bytes(100, 100, 20)
    fs, fq, ys, yq = LH.kernel_inputs(515, 36, 36, 40, 1)
    assert ys[0].tolist() == list(range(36)) and set(yq[0].tolist()) == set(range(36)) and 515 % 2 == 1 and 515 > 512
    assert LH.kernel_inputs(515, 5, 3, 75, 2)[2].tolist() == [[0, 2, 4]] * 2 and 75 > 64
    assert np.linalg.matrix_rank(LH.kernel_inputs(1, 5, 5, 5, 1)[0][0].astype(np.float64) @ LH.kernel_inputs(1, 5, 5, 5, 1)[0][0].astype(np.float64).T) == 1
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    assert re.search(r'#define MI_RIDGE_MAX_FEAT %d\b' % LH.MAX_FEAT, header)
    assert '8 * (ns * ns + nq * ns + 10 * ns * ways + nq * ways + 2 * ns + 3 * nq + 32) <= 163840' in header
    kernel = open(os.path.join(REPO, 'exploring_meta_amd', 'csrc', 'logreg_head.hip')).read()
    assert 'kStop = 1e-13, kAccept = 1e-10, kCgTol2 = 1e-26, kArmijo = 1e-4' in kernel
    assert (LH.STOP, LH.ACCEPT, LH.CG_TOL ** 2, LH.ARMIJO) == (1e-13, 1e-10, 1e-26, 1e-4)


def test_symbols_declared_and_bound():
    symbols_declared_and_bound(SYMBOLS)


def test_driver_flags():
    from exploring_meta_amd.vision import anil_vision, logreg_vision, maml_vision
    p = logreg_vision.build_parser().parse_args([])
    assert p.lam == 1.0 and p.scale == 1.0 and p.dataset == 'min' and p.save_dir == '' and p.fix_head is False
    p = logreg_vision.build_parser().parse_args(['--dataset', 'omni', '--lam', '50', '--scale', '2', '--fix_head', '--save_dir', 'x'])
    assert p.lam == 50.0 and p.scale == 2.0 and p.dataset == 'omni' and p.save_dir == 'x' and p.fix_head is True
    for mod in (anil_vision, maml_vision):
        args = mod.build_parser().parse_args([])
        assert not args.logreg_test and mod.params_of(args)['logreg_test'] is False
        args = mod.build_parser().parse_args(['--logreg_test', '--logreg_lam', '50', '--logreg_scale', '2'])
        q = mod.params_of(args)
        assert q['logreg_test'] is True and q['logreg_lam'] == 50.0 and q['logreg_scale'] == 2.0 and q['ridge_test'] is False


def test_logreg_head_module():
    head = cf.LogRegHead(lam=50.0, scale=2.0)
    names = [n for n, _ in head.named_parameters()]
    assert names == ['log_lam', 'log_scale'] and all(p.dim() == 0 and p.requires_grad for p in head.parameters())
    assert head.lam == pytest.approx(50.0, rel=1e-6) and head.scale == pytest.approx(2.0, rel=1e-6)
    fixed = cf.LogRegHead(lam=50.0, scale=2.0, learnable=False)
    assert list(fixed.parameters()) == [] and sorted(fixed.state_dict()) == ['log_lam', 'log_scale']
    assert fixed.lam == pytest.approx(50.0, rel=1e-6) and fixed.scale == pytest.approx(2.0, rel=1e-6)
    fixed.load_state_dict(head.state_dict())                             # the two scalars travel between the two forms


def test_the_surface_refuses_without_a_gpu():
    """lam or scale <= 0 or not finite, another head's module and an OmniglotCNN are refused before anything touches a device."""
    trunk = torch.nn.Sequential(cf.ConvBase(output_size=32, hidden=32, channels=1, max_pool=False))
    data, labels = torch.zeros(1, 10, 1, 28, 28), torch.zeros(1, 10, dtype=torch.int64)

    class Tasks:
        def sample(self):
            raise AssertionError('refused before a task is drawn')
    p = dict(meta_batch_size=2, shots=1, ways=5)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(_lib.MiError, match='lam must be positive'):
            cf.LogRegHead(lam=bad)
        with pytest.raises(_lib.MiError, match='scale must be positive'):
            cf.LogRegHead(scale=bad)
    for name, text in (('log_lam', 'lam must be positive'), ('log_scale', 'scale must be positive')):
        head = cf.LogRegHead()
        with torch.no_grad():
            getattr(head, name).fill_(float('nan'))                      # (an optimiser step gone wrong)
        with pytest.raises(_lib.MiError, match=text):
            cf.meta_batch_adapt_logreg(trunk, head, data, labels, 1, 5)
        with pytest.raises(_lib.MiError, match=text):
            cf.fast_adapt_logreg((data[0], labels[0]), trunk, head, 1, 5, 'cpu')
        with pytest.raises(_lib.MiError, match=text):
            cf.evaluate_logreg(p, Tasks(), trunk, head, 'cpu')
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.evaluate_logreg(p, Tasks(), cf.OmniglotCNN(5), cf.LogRegHead(), 'cpu')
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.meta_batch_adapt_logreg(cf.OmniglotCNN(5), cf.LogRegHead(), data, labels, 1, 5)
    for other in (torch.nn.Linear(32, 5), cf.RidgeHead()):
        with pytest.raises(TypeError, match='LogRegHead'):
            cf.meta_batch_adapt_logreg(trunk, other, data, labels, 1, 5)
    from exploring_meta_amd.engine import MetaEngine, check_logreg
    assert callable(MetaEngine.meta_batch_logreg) and callable(MetaEngine.logreg_head)
    assert check_logreg(2, 3) == (2.0, 3.0) and math.isfinite(cf.LogRegHead(1e-3, 1e3).lam)
