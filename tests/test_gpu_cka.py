"""CKA on the GPU (csrc/cka.hip through mi_cka and exploring_meta_amd/utils/cka.py) against the reference's own results
(golden_cka.npz), the fp64 restatement (tests/cka_oracle.py), invariances, real representations of a Mini-ImageNet learner and
the representation-change loop (misc_scripts/rc_vision.py: run_rep_cka)."""
import os

import numpy as np
import pytest
import torch

import cka_oracle as O
from gpu_utils import report

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-6       # |delta CKA| and relative sigma^2 (fp32 distances and kernel entries, fp64 sums): measured 2.6e-8 and 8.2e-8


def _cka(x, y, sigma=None):
    from exploring_meta_amd.utils.cka import cka
    return cka(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), sigma)


def _row(r, k=0):
    return np.array([float(r.linear[k]), float(r.kernel[k]), float(r.sigma_x[k]), float(r.sigma_y[k])])


def _check(got, want, tol=TOL):
    """got, want: (linear, kernel, sigma_x, sigma_y); sigma compared as sigma^2, relative"""
    err_cka = max(abs(got[0] - want[0]), abs(got[1] - want[1]))
    err_sig = max(abs(got[2] ** 2 - want[2] ** 2) / want[2] ** 2, abs(got[3] ** 2 - want[3] ** 2) / want[3] ** 2)
    assert err_cka <= tol and err_sig <= tol, (got, want)
    return err_cka, err_sig


def test_cka_matches_reference_records_and_oracle():
    g = np.load(os.path.join(HERE, 'golden', 'golden_cka.npz'), allow_pickle=False)
    worst = [0.0, 0.0, 0.0, 0.0]
    for idx, (kind, seed, n, p, sigma) in enumerate(O.CASES):
        x, y = O.make_case(kind, seed, n, p)
        s = sigma if sigma > 0 else None
        got = _row(_cka(x, y, s))
        e = _check(got, g['result'][idx])
        o = O.cka(x, y, s)
        e2 = _check(got, (o['linear'], o['kernel'], o['sigma_x'], o['sigma_y']))
        worst = [max(a, b) for a, b in zip(worst, e + e2)]
    report('cka_golden_and_oracle', golden_cka=worst[0], golden_sigma2=worst[1], oracle_cka=worst[2], oracle_sigma2=worst[3])


def test_cka_invariances_and_degenerate_cases():
    x, _ = O.make_case('relu', 21, 900, 25)
    r = _row(_cka(x, x))
    assert abs(r[0] - 1) <= 1e-12 and abs(r[1] - 1) <= 1e-12 and r[2] == r[3]
    # Y = c X Q, Q orthogonal: both CKAs are 1 (the median bandwidth scales with c)
    q, _ = np.linalg.qr(O.make_case('gauss', 22, 25, 25)[0].astype(np.float64))
    y = (3.0 * x.astype(np.float64) @ q).astype(np.float32)
    r = _row(_cka(x, y))
    assert abs(r[0] - 1) <= 1e-5 and abs(r[1] - 1) <= 1e-5 and abs(r[3] / r[2] - 3.0) <= 1e-5
    # NaN exactly where numpy gives NaN: all rows identical (empty median), constant X (0 / 0)
    ones = np.ones((50, 4), np.float32)
    z = O.make_case('gauss', 23, 50, 4)[0]
    for a, b, s in ((ones, z, None), (z, ones, None), (ones, z, 1.0), (ones, ones, None)):
        got, want = _row(_cka(a, b, s)), O.cka(a, b, s)
        assert list(np.isnan(got)) == [bool(np.isnan(want[k])) for k in ('linear', 'kernel', 'sigma_x', 'sigma_y')], (got, want)


def test_cka_is_deterministic_and_independent_of_the_batch():
    xs = torch.stack([torch.from_numpy(O.make_case('relu', 30 + k, 700, 25)[0]) for k in range(8)]).cuda()
    ys = torch.stack([torch.from_numpy(O.make_case('relu', 30 + k, 700, 25)[1]) for k in range(8)]).cuda()
    a, b = _cka(xs, ys), _cka(xs, ys)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    alone = _cka(xs[3], ys[3])
    for u, v in zip(a, alone):
        assert torch.equal(u[3:4], v)


@pytest.fixture(scope='module')
def mini_reps():
    """Reps of a Mini-ImageNet 5-way 5-shot learner's adaptation data before and after one adapt step, layers 0-4 and -1, as the
    [c*h*w, b] matrices of rc_vision (the logits [b, ways] as they are)."""
    from exploring_meta_amd import core_functions as cf
    from exploring_meta_amd.misc_scripts import rc_vision
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    torch.manual_seed(0)
    maml = cf.MAML(cf.MiniImagenetCNN(5).cuda(), lr=0.1)
    init, learner = maml.clone(), maml.clone()
    dev = torch.device('cuda')
    ad, al, _, _ = cf.prepare_batch(SyntheticTasks('min', 5, 5, 7).sample(), 5, 5, dev)
    learner.adapt(torch.nn.CrossEntropyLoss()(learner(ad), al) / len(ad))
    return {layer: (rc_vision._device_rep(learner, ad, layer), rc_vision._device_rep(init, ad, layer)) for layer in (0, 1, 2, 3, 4, -1)}


def test_cka_of_real_representations(mini_reps):
    shapes = {k: tuple(v[0].shape) for k, v in mini_reps.items()}
    assert shapes == {0: (21168, 25), 1: (56448, 25), 2: (14112, 25), 3: (3200, 25), 4: (800, 25), -1: (25, 5)}
    r0 = _row(_cka(*mini_reps[0]))
    assert abs(r0[0] - 1) <= 1e-12 and abs(r0[1] - 1) <= 1e-12          # layer 0 is the same input on both sides
    worst = 0.0
    for layer in (2, 3, 4, -1):
        a, b = mini_reps[layer]
        got = _row(_cka(a, b))
        o = O.cka(a.cpu().numpy(), b.cpu().numpy())
        worst = max(worst, *_check(got, (o['linear'], o['kernel'], o['sigma_x'], o['sigma_y'])))
    report('cka_real_reps', worst=worst)


def _blocks(n, bs=128):
    # (torch.cdist's direct-difference kernel launches one workgroup of 256 threads per output: past 2^32 threads per launch its
    # results were wrong on ROCm, so blocks of rows stay below 2^32 / (256 n))
    return [(i0, min(i0 + bs, n)) for i0 in range(0, n, bs)]


def test_cka_full_size_layer1(mini_reps):
    """n = 56448: the engine's sigma^2 brackets the two middle ranks of the nonzero fp64 distances, and kernel CKA recomputed
    blockwise in fp64 from the engine's sigma agrees."""
    a, b = (m.double() for m in mini_reps[1])
    n = a.shape[0]
    r = _row(_cka(*mini_reps[1]))
    cols = torch.arange(n, device='cuda')

    def dist(m, i0, i1):
        return torch.cdist(m[i0:i1], m, compute_mode='donot_use_mm_for_euclid_dist') ** 2

    for m, sig in ((a, r[2]), (b, r[3])):
        s2 = sig * sig
        M = lo = hi = 0
        for i0, i1 in _blocks(n):
            d = dist(m, i0, i1)
            upper = cols[None, :] > torch.arange(i0, i1, device='cuda')[:, None]
            d = d[upper & (d != 0)]
            M += d.numel()
            lo += int((d < s2 * (1 - 1e-5)).sum())
            hi += int((d <= s2 * (1 + 1e-5)).sum())
        assert lo <= (M - 1) // 2 and hi >= M // 2 + 1, (M, lo, hi)
    cs = []
    for m, sig in ((a, r[2]), (b, r[3])):
        rs = torch.cat([torch.exp(-dist(m, i0, i1) / (2 * sig * sig)).sum(1) for i0, i1 in _blocks(n)])
        cs.append(rs / n - rs.sum() / (2.0 * n * n))
    h = torch.zeros(3, dtype=torch.float64, device='cuda')
    for i0, i1 in _blocks(n):
        cx = torch.exp(-dist(a, i0, i1) / (2 * r[2] ** 2)) - cs[0][i0:i1, None] - cs[0][None, :]
        cy = torch.exp(-dist(b, i0, i1) / (2 * r[3] ** 2)) - cs[1][i0:i1, None] - cs[1][None, :]
        h += torch.stack([(cx * cy).sum(), (cx * cx).sum(), (cy * cy).sum()])
    want = float(h[0] / torch.sqrt(h[1] * h[2]))
    assert abs(r[1] - want) <= TOL
    ac, bc = a - a.mean(0), b - b.mean(0)
    hl = lambda u, v: float(((u.T @ v) ** 2).sum())         # noqa: E731
    assert abs(r[0] - hl(ac, bc) / np.sqrt(hl(ac, ac) * hl(bc, bc))) <= 1e-9
    report('cka_layer1_full_size', kernel_err=abs(r[1] - want), sigma_x=r[2], sigma_y=r[3])


def test_run_rep_cka_matches_per_pair_calls():
    from exploring_meta_amd import core_functions as cf
    from exploring_meta_amd.misc_scripts import rc_vision
    from exploring_meta_amd.utils.cka import get_kernel_CKA, get_linear_CKA
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    torch.manual_seed(0)
    maml = cf.MAML(cf.MiniImagenetCNN(5).cuda(), lr=0.1)
    loss = torch.nn.CrossEntropyLoss(reduction='mean')
    dev = torch.device('cuda')
    params = dict(adapt_steps=1, inner_lr=0.1, n_tasks=2, layers=[0, 1, 4, -1])
    acc, res = rc_vision.run_rep_cka(maml, loss, SyntheticTasks('min', 5, 5, 60), dev, 5, 5, params)
    acc2, reps = rc_vision.run_rep_exp(maml, loss, SyntheticTasks('min', 5, 5, 60), dev, 5, 5, params)
    assert acc.shape == (2, 2) and np.array_equal(acc, acc2)
    assert set(res) == {'linear', 'kernel'} and set(res['linear']) == set(res['kernel']) == {0, 1, 4, -1}
    for kind, fn in (('linear', get_linear_CKA), ('kernel', get_kernel_CKA)):
        for layer, vals in res[kind].items():
            assert len(vals) == 2 and all(-1e-9 <= v <= 1 + 1e-9 for v in vals), (kind, layer, vals)
            if layer == 0:
                assert vals == [1.0, 1.0]
            for t, (ra, ri) in enumerate(reps[layer]):
                assert abs(vals[t] - fn(ra, ri)) <= 1e-9, (kind, layer, t)
