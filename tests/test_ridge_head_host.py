"""CPU tests of the ridge-regression head: the closed form the kernel implements against fp64 autograd of the
definition (tests/ridge_head_oracle.py), the omitted bias, the conditions the GPU test puts on its fused-call inputs, the kernel's
square-root-free factor and substitution loops restated in numpy, the drivers' flags, the C symbols, and what the Python surface refuses
without a GPU; the bar that holds the kernel to its fp64 claim (ridge_head_oracle.tight_errors, against the closed form in np.longdouble):
the reference itself, an fp64 model of the kernel inside it, the same model with an fp32 Gram matrix outside it, and the conditions the edge
cases and the pivot case of the GPU test rest on."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
import ridge_head_oracle as RH
from closed_form_utils import symbols_declared_and_bound

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('mi_ridge_head_scratch_bytes', 'mi_ridge_head', 'mi_ridge_workspace_bytes', 'mi_meta_batch_ridge')
NAMES = ('loss', 'acc', 'logits', 'dfs', 'dfq', 'dhyper')


# (33, 3, 6, 4): unbalanced classes (counts 1, 2, 3) and ns != nq; (16, 5, 5, 7): ns != nq; (128, 1, 3, 3): one class; (1, 5, 5, 5): G has
# rank one before lam I
@pytest.mark.parametrize('lam,alpha', [(1.0, 8.0), (50.0, 8.0), (0.5, 1.5)])
@pytest.mark.parametrize('feat,ways,ns,nq,T', [(33, 3, 6, 4, 2), (16, 5, 5, 7, 1), (128, 1, 3, 3, 1), (1, 5, 5, 5, 1)])
def test_closed_form_is_autograd(feat, ways, ns, nq, T, lam, alpha):
    """Loss, logits, dfs, dfq, dlam and dalpha of the closed form = fp64 autograd through torch.linalg.solve to 1e-10."""
    fs, fq, ys, yq = RH.kernel_inputs(feat, ways, ns, nq, T)
    if (ways, ns) == (3, 6):
        assert sorted(np.bincount(ys[0], minlength=ways)) == [1, 2, 3]
    want = RH.head(fs, fq, ys, yq, ways, lam, alpha)
    got = RH.closed_form(fs, fq, ys, yq, ways, lam, alpha)
    assert np.allclose(got[1], want[1], rtol=0, atol=1e-6)                 # (the oracle's accuracy is vision_ref's fp32 ratio)
    for name, a, b in zip(NAMES, got, want[:6]):
        if name == 'acc':
            continue
        assert a.shape == b.shape and (RH.rel_err(a, b) < 1e-10 or (np.abs(b).max() == 0 and np.abs(a).max() < 1e-300)), (name, RH.rel_err(a, b))
    if ways > 1:
        assert np.abs(want[3]).sum() > 0 and np.abs(want[4]).sum() > 0 and np.all(want[5] != 0)
    else:
        assert np.all(want[0] == 0) and np.all(want[5] == 0)


def test_the_omitted_bias_has_no_gradient():
    """R2-D2's additive logit bias: every row of dz sums to 0, so d loss / d beta is 0 (to rounding) -- the head leaves it out."""
    for feat, ways, ns, nq, T in [(33, 3, 6, 4, 2), (16, 5, 5, 7, 1)]:
        fs, fq, ys, yq = RH.kernel_inputs(feat, ways, ns, nq, T)
        assert abs(RH.bias_gradient(fs, fq, ys, yq, ways, 1.0, 8.0)) < 1e-14


def _ldl_solve(g, x):
    """The kernel's loops in numpy, fp64: G = L D L^T in place on the lower triangle (column j keeps L D, the diagonal D), then forward,
    diagonal and backward substitution on X in place, every step reading one row of X and writing the others."""
    g, x = np.tril(g).copy(), x.copy()
    n = g.shape[0]
    invd = np.zeros(n)
    for j in range(n):
        assert g[j, j] > 0
        invd[j] = 1.0 / g[j, j]
        for i in range(j + 1, n):
            lij = g[i, j] * invd[j]
            for k in range(j + 1, i + 1):
                g[i, k] -= lij * g[k, j]
    for k in range(n - 1):
        for i in range(k + 1, n):
            x[i] -= (g[i, k] * invd[k]) * x[k]
    x *= invd[:, None]
    for k in range(n - 1, 0, -1):
        for i in range(k):
            x[i] -= (g[k, i] * invd[i]) * x[k]
    return x


@pytest.mark.parametrize('n,feat,lam', [(1, 4, 1.0), (7, 3, 0.5), (25, 64, 1.0), (40, 1, 50.0)])
def test_the_kernels_factor_and_substitution(n, feat, lam):
    """The square-root-free Cholesky and the one-barrier-per-column substitutions of csrc/ridge_head.hip solve G X = Y: against
    numpy.linalg.solve to 1e-11 (cond(G) <= 160 at these sizes), and scaling G by 4 scales the solution by 1/4 exactly."""
    fs = RH.kernel_inputs(feat, 1, n, n, 1)[0][0].astype(np.float64)
    g = fs @ fs.T + lam * np.eye(n)
    y = np.eye(n)[:, :max(1, n // 2)]
    x = _ldl_solve(g, y)
    assert RH.rel_err(x, np.linalg.solve(g, y)) < 1e-11
    assert np.array_equal(_ldl_solve(4 * g, y), x / 4)


@functools.lru_cache(maxsize=None)
def _oracle(shape):
    return RH.case_oracle(shape)


@pytest.mark.parametrize('shape', list(RH.FUSED_CASES))
def test_oracle_conditions_of_the_gpu_cases(shape):
    """What the GPU test needs of its fused-call inputs, met by the fp64 reference alone: every task's loss inside [0.05, 3] (neither
    saturated nor untrained), at most one query row in ten of a task under the accuracy margin, and gradients that are not zero."""
    ids = RH.FUSED_CASES[shape][0]
    ways, shots = RH.SHAPES[shape][4:]
    o = _oracle(shape)
    clear = RH.clear_rows(o['logits'][None])[0]
    print(f'[ridge cases] {shape} (lam, alpha) = {RH.FUSED_CASES[shape][1:]}: losses {o["losses"]}, accs {o["accs"]}, '
          f'unclear rows per task {(~clear).sum(axis=-1)}, dhyper {o["dhyper"].tolist()}')
    assert clear.shape == (len(ids), ways * shots)
    assert np.all((~clear).sum(axis=-1) * 10 <= ways * shots), (~clear).sum(axis=-1)
    assert np.all(o['losses'] >= 0.05) and np.all(o['losses'] <= 3.0), o['losses']
    assert np.abs(o['grad_feat']).sum() > 0 and np.all(o['dhyper'] != 0)


def test_kernel_cases_and_the_domain():
    """The kernel-entry cases are metric_head_oracle's and Omniglot 20-way 5-shot; every one is inside the LDS inequality of the header,
    the largest with 240 bytes to spare."""
    assert RH.KERNEL_CASES[:-1] == list(RH.M.KERNEL_CASES) and RH.KERNEL_CASES[-1] == (128, 20, 100, 100, 1)
    assert RH.HYPERS == [(1.0, 8.0), (50.0, 8.0)]
    for feat, ways, ns, nq, T in RH.KERNEL_CASES:
        assert RH.lds_bytes(ns, nq, ways) <= 163840 and feat <= RH.MAX_FEAT
    assert RH.lds_bytes(100, 100, 20) == 163600
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    assert re.search(r'#define MI_RIDGE_MAX_FEAT %d\b' % RH.MAX_FEAT, header)
    assert '8 * (ns (ns + 1) / 2 + nq * ns + 2 * ns * ways + ns + 3 * nq) + 4 * nq * ways <= 163840' in header


# ---------------------------------------------------------------------------------------------------------------- the fp64 claim's bar
# Fail loudly, never skip: without an extended format the reference is no better than what it judges.
assert np.finfo(np.longdouble).eps <= 2.0 ** -63, 'np.longdouble must be the 80-bit extended format (eps 2^-63) for the ridge reference'

# every case the GPU test sends through _check_kernel: the kernel cases, the edge cases, and test_domain_limits' feat = MI_RIDGE_MAX_FEAT
BAR_CASES = [c + h for c in RH.KERNEL_CASES + RH.EDGE_CASES for h in RH.HYPERS] + [(RH.MAX_FEAT, 5, 5, 5, 1, 1.0, 8.0)]
BAR_IDS = ['-'.join(f'{v:g}' for v in c) for c in BAR_CASES]


@functools.lru_cache(maxsize=None)
def _o64(case):
    """(inputs, fp64 autograd oracle) of a BAR_CASES entry, shared by the tests below (never modified)."""
    feat, ways, ns, nq, T, lam, alpha = case
    inputs = RH.kernel_inputs(feat, ways, ns, nq, T)
    return inputs, RH.head(*inputs, ways, lam, alpha, torch.float64)


def _model(case, **kw):
    """The kernel's arithmetic as the header states it, in NumPy: fp64 sums, factor and solves, dP and every output rounded to fp32."""
    (fs, fq, ys, yq), _ = _o64(case)
    return RH.closed_form_np(fs, fq, ys, yq, case[1], case[5], case[6], np.float64, round_dp=True, round_out=True, **kw)


def _tight(case, got):
    (fs, fq, ys, yq), o64 = _o64(case)
    return RH.tight_errors(got, o64, fs, fq, ys, yq, case[1], case[5], case[6])


@pytest.mark.parametrize('case', BAR_CASES, ids=BAR_IDS)
def test_extended_reference_is_the_closed_form(case):
    """closed_form_ext (np.longdouble, hand-written L D L^T) = closed_form (fp64, LAPACK) to 1e-9 wherever cond_2(G) < 1e3, and rounding dP
    to fp32 moves loss, logits and dalpha by nothing at all."""
    (fs, fq, ys, yq), o64 = _o64(case)
    ways, lam, alpha = case[1], case[5], case[6]
    ext, ext_dp = (RH.quantities(RH.closed_form_ext(fs, fq, ys, yq, ways, lam, alpha, r)) for r in (False, True))
    for n in ('loss', 'logits', 'dalpha'):
        assert np.array_equal(ext[n], ext_dp[n]), n
    if o64[6].max() < 1e3:
        want = RH.quantities(RH.closed_form(fs, fq, ys, yq, ways, lam, alpha))
        for n in RH.QUANTITIES:
            assert ext[n].shape == want[n].shape and RH.rel_ext(want[n], ext[n]) < 1e-9, (n, RH.rel_ext(want[n], ext[n]))
        acc = RH.closed_form_ext(fs, fq, ys, yq, ways, lam, alpha, False)[1]
        assert np.allclose(acc.astype(np.float64), o64[1], rtol=0, atol=1e-6)  # (the oracle's accuracy is vision_ref's fp32 ratio)


def test_extended_reference_was_compared_somewhere():
    assert sum(float(_o64(c)[1][6].max()) < 1e3 for c in BAR_CASES) >= len(BAR_CASES) // 2


@pytest.mark.parametrize('case', BAR_CASES, ids=BAR_IDS)
def test_the_kernels_model_stays_inside_the_tight_bar(case):
    """The reference alone stays within it: fp64 arithmetic with fp32 dP and fp32 stores meets 2^-23 + 2 e_dp + 2 e64 on every quantity
    and on every row of logits, dfs and dfq."""
    res = _tight(case, _model(case))
    print(f'[tight bar, model] {case}: ' + ', '.join(f'{n} {np.max(e):.2e} ({np.max(e / b):.2f} of its bar)' for n, (e, b) in res.items()))
    for n, (err, bar) in res.items():
        assert np.all(err <= bar), (n, np.max(err / bar))


@pytest.mark.parametrize('case', [c for c in BAR_CASES if c[2] >= 20], ids=[i for c, i in zip(BAR_CASES, BAR_IDS) if c[2] >= 20])
def test_an_fp32_gram_matrix_breaks_the_tight_bar(case):
    """The bar has teeth: the same model with Fs Fs^T accumulated in fp32 -- the regression the header rules out -- is rejected on logits,
    dfs and dfq in every case with ns >= 20."""
    res = _tight(case, _model(case, gram_dtype=np.float32))
    print(f'[tight bar, fp32 Gram] {case}: ' + ', '.join(f'{n} {np.max(e):.2e} ({np.max(e / b):.2f} of its bar)' for n, (e, b) in res.items()))
    for n in RH.ROWWISE:
        assert res[n][0] > res[n][1], (n, res[n])


@pytest.mark.parametrize('case', [c + h for c in RH.EDGE_CASES for h in RH.HYPERS])
def test_edge_cases_meet_the_conditions_the_gpu_test_rests_on(case):
    """Settled on the fp64 reference alone.  ways > 1: every task's loss above 1e-3 and no gradient zero, so a relative bar means
    something; every row's top-2 logit margin is at least 10 x what the tight bar lets two returned logits move against each other (twice
    the row's bar times the row's norm; 1 x would do), so `argmax equal on every row` cannot turn on a rounding."""
    (fs, fq, ys, yq), o64 = _o64(case)
    ways = case[1]
    if ways == 1:
        assert np.all(o64[0] == 0) and np.all(o64[5] == 0)
        return
    assert np.all(o64[0] > 1e-3) and np.abs(o64[3]).sum() > 0 and np.abs(o64[4]).sum() > 0 and np.all(o64[5] != 0), (o64[0], o64[5])
    bar = RH.tight_errors(o64, o64, fs, fq, ys, yq, ways, case[5], case[6])['logits_rows'][1]
    z = o64[2].reshape(-1, ways)
    top2 = np.sort(z, axis=-1)[:, -2:]
    margin, moves = top2[:, 1] - top2[:, 0], 2 * bar * np.linalg.norm(z, axis=-1)
    print(f'[edge case] {case}: loss {o64[0]}, smallest margin {margin.min():.3e}, largest move {moves.max():.3e}')
    assert np.all(margin > 10 * moves), (margin.min(), moves.max())


def test_edge_cases_take_the_paths_they_are_there_for():
    """Every edge case is inside the header's LDS inequality; the 64-way one asks for 138128 bytes, above the 64 KiB a kernel gets without
    the dynamic-LDS attribute, and its query labels reach lanes 32 to 63; 515 is odd and above one trip of the 512 threads; (5 ways, 3
    rows) has classes 1 and 3 without a support row and nq > 64."""
    assert RH.EDGE_CASES == [(515, 64, 64, 70, 1), (515, 5, 3, 75, 2), (4, 2, 1, 1, 1), (5, 1, 1, 3, 1)]
    for feat, ways, ns, nq, T in RH.EDGE_CASES:
        assert RH.lds_bytes(ns, nq, ways) <= 163840 and feat <= RH.MAX_FEAT
    assert RH.lds_bytes(64, 70, 64) == 138128 > 64 * 1024
    fs, fq, ys, yq = RH.kernel_inputs(515, 64, 64, 70, 1)
    assert set(yq[0].tolist()) == set(range(64)) and ys[0].tolist() == list(range(64))
    assert RH.kernel_inputs(515, 5, 3, 75, 2)[2].tolist() == [[0, 2, 4]] * 2 and 75 > 64 and 515 % 2 == 1 and 515 > 512


@pytest.mark.parametrize('plant_nan', [False, True])
def test_the_pivot_case_has_one_bad_task(plant_nan):
    """lam = 2^-80 is a positive normal fp32; in fp64 task 1's pivots are exactly (4, 0) (NaN with a NaN planted), those of tasks 0 and 2
    are positive by a wide margin, and their results are finite."""
    fs, fq, ys, yq = RH.pivot_inputs(plant_nan)
    lam = np.float32(RH.PIVOT_LAM)
    assert lam > 0 and np.isfinite(lam) and float(lam) == RH.PIVOT_LAM and lam >= np.finfo(np.float32).tiny
    for t in range(3):
        s = fs[t].astype(np.float64)
        _, d = RH.ldl(s @ s.T + float(lam) * np.eye(2))
        if t == 1:
            assert d[0] == 4.0 or plant_nan
            assert not d[1] > 0 and (plant_nan or d[1] == 0.0), d
        else:
            assert np.all(d > 1e-2), d
    good = RH.closed_form_np(fs[::2], fq[::2], ys[::2], yq[::2], 2, lam, 8.0)
    assert all(np.isfinite(g).all() for g in good)


def test_symbols_declared_and_bound():
    symbols_declared_and_bound(SYMBOLS)
    # the metric entries keep their two metrics: the ridge head has entries of its own
    from exploring_meta_amd.engine import METRICS
    assert METRICS == {'proto': 0, 'cosine': 1}


def test_driver_flags():
    from exploring_meta_amd.vision import anil_vision, maml_vision, ridge_vision
    p = ridge_vision.build_parser().parse_args([])
    assert p.lam == 1.0 and p.scale == 1.0 and p.dataset == 'min' and p.save_dir == '' and p.fix_head is False
    p = ridge_vision.build_parser().parse_args(['--dataset', 'omni', '--lam', '50', '--scale', '8', '--fix_head', '--save_dir', 'x'])
    assert p.lam == 50.0 and p.scale == 8.0 and p.dataset == 'omni' and p.save_dir == 'x' and p.fix_head is True
    for mod in (anil_vision, maml_vision):
        args = mod.build_parser().parse_args([])
        assert not args.ridge_test and mod.params_of(args)['ridge_test'] is False
        args = mod.build_parser().parse_args(['--ridge_test', '--ridge_lam', '50', '--ridge_scale', '8'])
        q = mod.params_of(args)
        assert q['ridge_test'] is True and q['ridge_lam'] == 50.0 and q['ridge_scale'] == 8.0


def test_ridge_head_module():
    head = cf.RidgeHead(lam=50.0, scale=8.0)
    names = [n for n, _ in head.named_parameters()]
    assert names == ['log_lam', 'log_scale'] and all(p.dim() == 0 and p.requires_grad for p in head.parameters())
    assert head.lam == pytest.approx(50.0, rel=1e-6) and head.scale == pytest.approx(8.0, rel=1e-6)
    fixed = cf.RidgeHead(lam=50.0, scale=8.0, learnable=False)
    assert list(fixed.parameters()) == [] and sorted(fixed.state_dict()) == ['log_lam', 'log_scale']
    assert fixed.lam == pytest.approx(50.0, rel=1e-6) and fixed.scale == pytest.approx(8.0, rel=1e-6)
    fixed.load_state_dict(head.state_dict())                             # the two scalars travel between the two forms


def test_the_surface_refuses_without_a_gpu():
    """lam or scale <= 0 or NaN and an OmniglotCNN are refused before anything touches a device."""
    trunk = torch.nn.Sequential(cf.ConvBase(output_size=32, hidden=32, channels=1, max_pool=False))
    data, labels = torch.zeros(1, 10, 1, 28, 28), torch.zeros(1, 10, dtype=torch.int64)

    class Tasks:
        def sample(self):
            raise AssertionError('refused before a task is drawn')
    p = dict(meta_batch_size=2, shots=1, ways=5)
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(_lib.MiError, match='lam must be positive'):
            cf.RidgeHead(lam=bad)
        with pytest.raises(_lib.MiError, match='scale must be positive'):
            cf.RidgeHead(scale=bad)
    for name, text in (('log_lam', 'lam must be positive'), ('log_scale', 'scale must be positive')):
        head = cf.RidgeHead()
        with torch.no_grad():
            getattr(head, name).fill_(float('nan'))                      # (an optimiser step gone wrong)
        with pytest.raises(_lib.MiError, match=text):
            cf.meta_batch_adapt_ridge(trunk, head, data, labels, 1, 5)
        with pytest.raises(_lib.MiError, match=text):
            cf.fast_adapt_ridge((data[0], labels[0]), trunk, head, 1, 5, 'cpu')
        with pytest.raises(_lib.MiError, match=text):
            cf.evaluate_ridge(p, Tasks(), trunk, head, 'cpu')
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.evaluate_ridge(p, Tasks(), cf.OmniglotCNN(5), cf.RidgeHead(), 'cpu')
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.meta_batch_adapt_ridge(cf.OmniglotCNN(5), cf.RidgeHead(), data, labels, 1, 5)
    with pytest.raises(TypeError, match='RidgeHead'):
        cf.meta_batch_adapt_ridge(trunk, torch.nn.Linear(32, 5), data, labels, 1, 5)
    from exploring_meta_amd.engine import MetaEngine, check_ridge
    assert callable(MetaEngine.meta_batch_ridge) and callable(MetaEngine.ridge_head)
    assert check_ridge(2, 3) == (2.0, 3.0) and math.isfinite(cf.RidgeHead(1e-3, 1e3).lam)
