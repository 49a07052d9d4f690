"""CCA on the GPU (csrc/cca.hip through mi_cca and exploring_meta_amd/utils/cca.py) against the reference's own results
(golden_cca.npz), the fp64 restatement (tests/cca_oracle.py), the degenerate rules, determinism, real representations of a
Mini-ImageNet learner and the representation-change loop (misc_scripts/rc_vision.py: run_rep_cca).

The bar of every comparison is cca_oracle.bar: max(1e-9, 1024 cond 2^-53), cond = max(cond_x, cond_y) taken from the golden file
(from the oracle where there is no golden record), never from the code under test.  Measured on an MI355X: 6.7e-13 at worst on
the well-conditioned cases (bar 1e-9), 3.1e-7 on dupcol at epsilon 1e-10 (bar 1.9e-3), 1.8e-13 on the real representations; at most
9 sweeps for the symmetric problems and 11 for the singular values."""
import os

import numpy as np
import pytest
import torch

import cca_oracle as O
from gpu_utils import report

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _cca(x, y, eps, detail=False):
    from exploring_meta_amd.utils.cca import cca
    return cca(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), eps, O.THRESHOLD, detail=detail)


def _mask(bits, p):
    return np.array([(int(bits) >> i) & 1 == 1 for i in range(p)], dtype=bool)


def _err(r, k, coefs, mean, tmean, total):
    """worst of |coefficients|, mean, thresholded mean and sum of pair k against the given values; the NaN padding must match"""
    got = r.coefs[k].cpu().numpy()
    count = int(r.count[k])
    assert count == len(coefs) and np.all(np.isnan(got[count:])) and np.all(np.isfinite(got[:count]))
    return max(np.abs(got[:count] - coefs).max(), abs(float(r.mean[k]) - mean), abs(float(r.thresholded_mean[k]) - tmean),
               abs(float(r.sum[k]) - total))


def _err_oracle(r, k, o):
    return _err(r, k, o['coefs'], o['mean'], o['thresholded_mean'], o['sum'])


def test_cca_matches_reference_records_and_oracle():
    g = np.load(os.path.join(HERE, 'golden', 'golden_cca.npz'), allow_pickle=False)
    worst_g = worst_o = worst_share = 0.0
    sweeps = np.zeros(3, dtype=np.int64)
    for idx, (kind, seed, n, p, eps) in enumerate(O.CASES):
        x, y = O.make_case(kind, seed, n, p)
        r, det = _cca(x, y, eps, detail=True)
        mean, tmean, total, cond_x, cond_y = g['stats'][idx]
        bar = O.bar(cond_x, cond_y)
        want = g['coefs'][idx]
        want = want[~np.isnan(want)]
        eg = _err(r, 0, want, mean, tmean, total)
        o = O.cca(x, y, eps, O.THRESHOLD)
        eo = _err_oracle(r, 0, o)
        print(f'[cca] {kind} {seed} n={n} p={p} eps={eps}: golden {eg:.2e} oracle {eo:.2e} bar {bar:.2e} '
              f'sweeps {det.sweeps[0].tolist()}', flush=True)
        assert eg <= bar and eo <= bar, (O.CASES[idx], eg, eo, bar)
        assert np.array_equal(_mask(det.x_mask[0], p), g['x_idxs'][idx, :p]) and np.array_equal(_mask(det.y_mask[0], p), g['y_idxs'][idx, :p])
        assert int(r.kept_x[0]) == o['kept_x'] and int(r.kept_y[0]) == o['kept_y'] and int(r.count[0]) == o['count']
        assert int(det.sweeps[0, 3]) == 0                                   # no sweep cap reached
        worst_g, worst_o, worst_share = max(worst_g, eg), max(worst_o, eo), max(worst_share, eg / bar, eo / bar)
        sweeps = np.maximum(sweeps, det.sweeps[0, :3].cpu().numpy())
    report('cca_golden_and_oracle', golden_err=worst_g, oracle_err=worst_o, worst_share_of_bar=worst_share,
           max_sweeps_sym=int(max(sweeps[:2])), max_sweeps_svd=int(sweeps[2]))


def test_cca_same_and_rotated():
    g = np.load(os.path.join(HERE, 'golden', 'golden_cca.npz'), allow_pickle=False)
    worst = 0.0
    for idx, (kind, seed, n, p, eps) in enumerate(O.CASES):
        if kind not in ('same', 'rot'):
            continue
        x, y = O.make_case(kind, seed, n, p)
        r = _cca(x, y, eps)
        o = O.cca(x, y, eps, O.THRESHOLD)
        bar = O.bar(*g['stats'][idx, 3:5])
        assert abs(o['mean'] - 1.0) <= 10 * max(eps, 1e-15)
        e = abs(float(r.mean[0]) - o['mean'])
        assert e <= bar, (kind, eps, e)
        worst = max(worst, e)
        if kind == 'same':
            assert float(r.kept_x[0]) == float(r.kept_y[0]) and float(r.cond_x[0]) == float(r.cond_y[0])
    report('cca_same_and_rotated', mean_err=worst)


def test_cca_degenerate_rules():
    ones = np.ones((50, 4), np.float32)
    z = O.make_case('gauss', 23, 50, 4)[0]
    for eps in (0.0, 1e-10):
        for a, b in ((ones, z), (z, ones), (ones, ones), (0.1 * ones, z)):
            r = _cca(a, b, eps)
            assert float(r.mean[0]) == float(r.thresholded_mean[0]) == float(r.sum[0]) == float(r.count[0]) == 0.0
            assert bool(torch.isnan(r.coefs).all())
    # epsilon = 0 with dead columns: finite, the cut directions add zero coefficients and count stays p
    x, y = O.make_case('dead', 9, 800, 25)
    r = _cca(x, y, 0.0)
    d = O.cca(np.delete(x, O.DEAD_X, axis=1), np.delete(y, O.DEAD_Y, axis=1), 0.0)
    got = r.coefs[0].cpu().numpy()
    assert int(r.count[0]) == int(r.kept_x[0]) == int(r.kept_y[0]) == 25 and np.all(np.isfinite(got))
    lead, total, tail = np.abs(got[:23] - d['coefs']).max(), abs(float(r.sum[0]) - d['sum']), np.abs(got[23:]).max()
    assert lead <= 1e-9 and total <= 1e-9 and tail <= 1e-9, (lead, total, tail)
    assert np.isinf(float(r.cond_x[0])) and np.isinf(float(r.cond_y[0]))
    report('cca_dead_columns_eps0', leading_err=lead, sum_err=total, trailing_max=tail)


def test_cca_is_deterministic_and_independent_of_the_batch():
    xs = torch.stack([torch.from_numpy(O.make_case('relu', 30 + k, 700, 25)[0]) for k in range(8)]).cuda()
    ys = torch.stack([torch.from_numpy(O.make_case('relu', 30 + k, 700, 25)[1]) for k in range(8)]).cuda()
    a, b = _cca(xs, ys, 1e-10), _cca(xs, ys, 1e-10)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    alone = _cca(xs[3], ys[3], 1e-10)
    for u, v in zip(a, alone):
        assert torch.equal(u[3:4], v)
    worst = 0.0
    for k in (0, 3, 7):
        o = O.cca(xs[k].cpu().numpy(), ys[k].cpu().numpy(), 1e-10, O.THRESHOLD)
        e = _err_oracle(a, k, o)
        assert e <= O.bar(o['cond_x'], o['cond_y'])
        worst = max(worst, e)
    report('cca_batch', oracle_err=worst)


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


def test_cca_of_real_representations(mini_reps):
    """Every layer, layer 0 (the same input on both sides) and the full-size layer 1 (n = 56448) included, against the oracle."""
    shapes = {k: tuple(v[0].shape) for k, v in mini_reps.items()}
    assert shapes == {0: (21168, 25), 1: (56448, 25), 2: (14112, 25), 3: (3200, 25), 4: (800, 25), -1: (25, 5)}
    worst = worst_share = 0.0
    means = {}
    for layer in (0, 1, 2, 3, 4, -1):
        a, b = mini_reps[layer]
        r, det = _cca(a, b, 1e-10, detail=True)
        o = O.cca(a.cpu().numpy(), b.cpu().numpy(), 1e-10, O.THRESHOLD)
        bar = O.bar(o['cond_x'], o['cond_y'])
        e = _err_oracle(r, 0, o)
        print(f'[cca] layer {layer}: err {e:.2e} bar {bar:.2e} cond {o["cond_x"]:.3g} {o["cond_y"]:.3g} mean {o["mean"]:.6f} '
              f'sweeps {det.sweeps[0].tolist()}', flush=True)
        assert e <= bar, (layer, e, bar)
        assert int(r.kept_x[0]) == o['kept_x'] and int(r.kept_y[0]) == o['kept_y'] and int(det.sweeps[0, 3]) == 0
        worst, worst_share = max(worst, e), max(worst_share, e / bar)
        means[f'mean_layer_{layer}'] = float(r.mean[0])
    report('cca_real_reps', worst=worst, worst_share_of_bar=worst_share, **means)


def test_run_rep_cca_matches_per_pair_calls():
    from exploring_meta_amd import core_functions as cf
    from exploring_meta_amd.misc_scripts import rc_vision
    from exploring_meta_amd.utils.cca import get_cca_similarity
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    torch.manual_seed(0)
    maml = cf.MAML(cf.MiniImagenetCNN(5).cuda(), lr=0.1)
    loss = torch.nn.CrossEntropyLoss(reduction='mean')
    dev = torch.device('cuda')
    params = dict(adapt_steps=1, inner_lr=0.1, n_tasks=2, layers=[0, 1, 4, -1])
    acc, res = rc_vision.run_rep_cca(maml, loss, SyntheticTasks('min', 5, 5, 60), dev, 5, 5, params)
    acc2, reps = rc_vision.run_rep_exp(maml, loss, SyntheticTasks('min', 5, 5, 60), dev, 5, 5, params)
    assert acc.shape == (2, 2) and np.array_equal(acc, acc2)
    assert set(res) == {0, 1, 4, -1}
    worst = 0.0
    for layer, vals in res.items():
        assert len(vals) == 2 and all(isinstance(v, float) and 0.0 <= v <= 1 + 1e-6 for v in vals), (layer, vals)
        for t, (ra, ri) in enumerate(reps[layer]):
            d, mean = get_cca_similarity(ra.T, ri.T, epsilon=1e-10)              # the reference's call (rc_vision.py:84-88)
            worst = max(worst, abs(vals[t] - mean))
            assert abs(vals[t] - mean) <= 1e-12, (layer, t, vals[t], mean)
            p = ra.shape[1]
            assert set(d) == {'cca_coef1', 'cca_coef2', 'mean', 'sum', 'x_idxs', 'y_idxs', 'idx1', 'idx2'}
            assert d['x_idxs'].dtype == bool and d['x_idxs'].shape == (p,) and d['y_idxs'].shape == (p,)
            s = d['cca_coef1']
            assert len(s) == min(d['x_idxs'].sum(), d['y_idxs'].sum()) and np.all(np.diff(s) <= 0)
            assert abs(mean - s.mean()) <= 1e-12 and abs(d['sum'][0] - s.sum()) <= 1e-12 and d['sum'][0] == d['sum'][1]
            assert d['idx1'] == d['idx2'] == O.threshold_index(s, 0.98)
            assert abs(d['mean'][0] - s[:d['idx1']].mean()) <= 1e-12 and d['mean'][0] == d['mean'][1]
    report('run_rep_cca', worst_vs_per_pair=worst)


# ------------------------------------------------------------------------------------------ the limits of the stated domain
# mi_maml.h: 1 <= p <= 64, 2 <= n <= 2^18, 1 <= pairs <= 2^20, epsilon >= 0, 0 <= threshold <= 1.  Inputs: cca_oracle.LIMIT_CASES /
# PAIR_CASES (their host side is tests/test_cca_host.py).

def _check_all(r, det, k, o, p):
    """Pair k of a detailed result against the oracle's dict: coefficients, the eight statistics, the kept masks, no sweep cap.
    The bar on the coefficients and the three means / sums is cca_oracle.bar with the ORACLE's condition numbers.  The condition
    numbers themselves: the smallest eigenvalue carries an absolute error of a few roundings of the largest, i.e. a relative error of
    that many roundings times cond -- the same quantity, so the same bar, taken relatively; inf and NaN must match as such."""
    bar = O.bar(o['cond_x'], o['cond_y']) if o['count'] else 1e-9
    stats = [float(v[k]) for v in (r.mean, r.thresholded_mean, r.sum, r.count, r.kept_x, r.kept_y, r.cond_x, r.cond_y)]
    assert stats[3:6] == [float(o['count']), float(o['kept_x']), float(o['kept_y'])], (stats, o)
    assert np.array_equal(_mask(det.x_mask[k], p), o['x_idxs']) and np.array_equal(_mask(det.y_mask[k], p), o['y_idxs'])
    assert int(det.sweeps[k, 3]) == 0, det.sweeps[k].tolist()
    got = r.coefs[k].cpu().numpy()
    count = o['count']
    assert np.all(np.isnan(got[count:])) and np.all(np.isfinite(got[:count]))
    err = 0.0
    if count:
        err = float(np.abs(got[:count] - o['coefs']).max())
    for g, w in zip(stats[:3], (o['mean'], o['thresholded_mean'], o['sum'])):
        assert np.isnan(g) == np.isnan(w), (stats, o)
        if not np.isnan(w):
            err = max(err, abs(g - w))
    assert err <= bar, (err, bar, stats)
    cerr = 0.0
    for g, w in zip(stats[6:], (o['cond_x'], o['cond_y'])):
        assert np.isnan(g) == np.isnan(w) and np.isinf(g) == np.isinf(w), (stats, o)
        if np.isfinite(w):
            cerr = max(cerr, abs(g - w) / w)
    assert cerr <= bar, (cerr, bar, stats)
    return err, cerr, bar


@pytest.mark.parametrize('idx', range(len(O.LIMIT_CASES)), ids=['{}-n{}-p{}-eps{}'.format(c[0], c[2], c[3], c[4]) for c in O.LIMIT_CASES])
def test_cca_at_the_limits_of_the_domain(idx):
    """Odd p at the LDS maximum (63; 64 with 63 x 61 kept), rectangular whitened blocks at p = 3 in both directions, p = 1, epsilon = 0,
    n < p, two row chunks, the chunk cap (n = 70001) and n = 2^18."""
    kind, seed, n, p, eps, zx, zy = O.LIMIT_CASES[idx]
    x, y = O.make_limit_case(kind, seed, n, p, zx, zy)
    r, det = _cca(x, y, eps, detail=True)
    o = O.cca(x, y, eps, O.THRESHOLD)
    assert (o['kept_x'], o['kept_y']) == (p - len(zx), p - len(zy))
    err, cerr, bar = _check_all(r, det, 0, o, p)
    report(f'cca_limit[{kind},n{n},p{p},eps{eps}]', err=err, cond_rel_err=cerr, bar=bar, sweeps=det.sweeps[0].tolist())


@pytest.mark.parametrize('threshold', [0.0, 1.0])
def test_cca_threshold_at_its_ends(threshold):
    """threshold = 0: the reference's sum_threshold returns index 0 (0 / sum >= 0) and np.mean of the empty prefix is NaN;
    threshold = 1: no proper prefix reaches the whole sum, every coefficient counts."""
    from exploring_meta_amd.utils.cca import cca, get_cca_similarity
    x, y = O.make_case('relu', 9, 800, 25)
    o = O.cca(x, y, 1e-10, threshold)
    idx, tmean = O.thresholded(o['coefs'], threshold)
    assert (idx, np.isnan(tmean)) == ((0, True) if threshold == 0.0 else (25, False)) and o['idx'] == idx
    r, det = cca(torch.as_tensor(x).cuda(), torch.as_tensor(y).cuda(), 1e-10, threshold, detail=True)
    err, cerr, bar = _check_all(r, det, 0, o, 25)
    got = float(r.thresholded_mean[0])
    assert np.isnan(got) if np.isnan(tmean) else abs(got - tmean) <= bar
    d, mean = get_cca_similarity(x.T, y.T, epsilon=1e-10, threshold=threshold)
    assert d['idx1'] == d['idx2'] == idx
    assert np.isnan(d['mean'][0]) if np.isnan(tmean) else abs(d['mean'][0] - tmean) <= bar
    assert abs(mean - o['mean']) <= bar
    report(f'cca_threshold[{threshold}]', err=err, idx=idx, thresholded_mean=got)


def test_cca_more_pairs_than_a_16_bit_grid_dimension():
    """pairs = 70000 > 65535: seven distinct 3 x 2 pairs (one keeps no neuron, one keeps 2 x 1) repeated cyclically; every row of the big
    call -- coefficients, statistics, kept masks, sweep counts -- must be the row of the 7-pair call bit for bit."""
    pairs, n, p, eps = 70000, 3, 2, 1e-6
    mats = [O.make_case(kind, seed, n, p) for kind, seed in O.PAIR_CASES]
    x7 = torch.from_numpy(np.stack([m[0] for m in mats])).cuda()
    y7 = torch.from_numpy(np.stack([m[1] for m in mats])).cuda()
    small, sdet = _cca(x7, y7, eps, detail=True)
    worst = 0.0
    for k, (xm, ym) in enumerate(mats):
        err, cerr, bar = _check_all(small, sdet, k, O.cca(xm, ym, eps, O.THRESHOLD), p)
        worst = max(worst, err / bar, cerr / bar)
    idx = torch.arange(pairs, device='cuda') % 7
    big, bdet = _cca(x7[idx].contiguous(), y7[idx].contiguous(), eps, detail=True)
    bits = lambda t: t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t           # noqa: E731  (NaN rows compare as bits)
    differing = 0
    for name, b, s in list(zip(small._fields, big, small)) + list(zip(sdet._fields, bdet, sdet)):
        same = bits(b) == bits(s[idx])
        differing += int((~same).sum())
        assert bool(same.all()), (name, (~same.reshape(pairs, -1).all(dim=1)).nonzero().flatten()[:8].tolist())
    report('cca_70000_pairs', worst_share_of_bar=worst, entries_differing=differing)
