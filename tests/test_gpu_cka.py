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


# ------------------------------------------------------------------------------------------ the limits of the stated domain
# mi_maml.h: 1 <= p <= 128, 2 <= n <= 2^18, pairs >= 1.  Inputs and expectations: cka_oracle.LIMIT_CASES / TIE_CASES (the host side
# of these checks is tests/test_cka_host.py).

_ORACLE = {}


def _oracle_row(kind, seed, n, p, sigma):
    """(linear, kernel, sigma_x, sigma_y) of the fp64 restatement, computed once per case"""
    key = (kind, seed, n, p, sigma)
    if key not in _ORACLE:
        x, y = O.make_case(kind, seed, n, p)
        with np.errstate(invalid='ignore', divide='ignore'):
            o = O.cka(x, y, sigma if sigma > 0 else None)
        _ORACLE[key] = np.array([o['linear'], o['kernel'], o['sigma_x'], o['sigma_y']], dtype=np.float64)
    return _ORACLE[key]


def _check_nan_aware(got, want, tol=TOL):
    """_check where the oracle is finite; NaN exactly where the oracle (numpy's rule) gives NaN.  -> (err_cka, err_sigma2)"""
    assert list(np.isnan(got)) == list(np.isnan(want)), (got, want)
    err_cka = max([abs(got[k] - want[k]) for k in (0, 1) if not np.isnan(want[k])], default=0.0)
    err_sig = max([abs(got[k] ** 2 - want[k] ** 2) / want[k] ** 2 for k in (2, 3) if not np.isnan(want[k])], default=0.0)
    assert err_cka <= tol and err_sig <= tol, (got, want, err_cka, err_sig)
    return err_cka, err_sig


@pytest.mark.parametrize('idx', range(len(O.LIMIT_CASES)), ids=['{}-n{}-p{}-s{}'.format(c[0], c[2], c[3], c[4]) for c in O.LIMIT_CASES])
def test_cka_at_the_limits_of_the_domain(idx):
    """p = 128 / 127, the histogram's 64 KiB LDS crossing (p = 96 -> 97), n = 2 and 3, the tile edge n = 63 / 64 / 65, the first column
    split n = 1025 and n = 2049, each with the median bandwidth; (130, 128) also with sigma = 2."""
    kind, seed, n, p, sigma = O.LIMIT_CASES[idx]
    x, y = O.make_case(kind, seed, n, p)
    got = _row(_cka(x, y, sigma if sigma > 0 else None))
    e = _check_nan_aware(got, _oracle_row(kind, seed, n, p, sigma))
    report(f'cka_limit[{kind},n{n},p{p},sigma{sigma}]', cka_err=e[0], sigma2_err=e[1])


def test_cka_median_of_heavily_tied_distances():
    """Rows on the lattice {0..3}^2: nine distinct squared distances, hundreds of ties, both middle ranks inside one radix bin or
    (the last two cases' X) on the two values 4 and 5.  Every distance is an exact small integer in fp32 and in fp64, so sigma^2 must
    be numpy's median exactly."""
    worst = 0.0
    for sx, sy, n, dup in O.TIE_CASES:
        x, y = O.lattice_rows(sx, n, dup), O.lattice_rows(sy, n, dup)
        got = _row(_cka(x, y))
        want2 = (O.exact_median_sigma2(x), O.exact_median_sigma2(y))
        print(f'[cka] lattice {sx} {sy} n={n}: sigma^2 {got[2] ** 2!r} {got[3] ** 2!r} want {want2}', flush=True)
        assert got[2] == np.sqrt(want2[0]) and got[3] == np.sqrt(want2[1]), (got, want2)          # the kernel's sqrt of the exact median
        o = O.cka(x, y)
        worst = max(worst, *_check(got, (o['linear'], o['kernel'], o['sigma_x'], o['sigma_y'])))
    report('cka_lattice_ties', worst=worst, sigma2_rel_err=0.0)


@pytest.mark.parametrize('kind,seed', [('gauss', 81), ('relu', 82)])
def test_cka_under_power_of_two_scaling(kind, seed):
    """(2^20 X, 2^-20 Y) against (X, Y): scaling by a power of two is exact in fp32, the distances scale by 2^40 / 2^-40 exactly, so
    the bandwidths scale by exactly 2^20 / 2^-20 and both CKAs stay within TOL of the oracle's value for (X, Y)."""
    x, y = O.make_case(kind, seed, 200, 5)
    base = _row(_cka(x, y))
    got = _row(_cka(x * np.float32(2.0 ** 20), y * np.float32(2.0 ** -20)))
    o = O.cka(x, y)
    e = _check(base, (o['linear'], o['kernel'], o['sigma_x'], o['sigma_y']))
    err = max(abs(got[0] - o['linear']), abs(got[1] - o['kernel']))
    assert err <= TOL, (got, o)
    assert got[2] / base[2] == 2.0 ** 20 and got[3] / base[3] == 2.0 ** -20, (got, base)
    report(f'cka_pow2_scaling[{kind}]', cka_err=err, unscaled_cka_err=e[0], cka_bit_identical=bool(got[0] == base[0] and got[1] == base[1]),
           linear_delta=abs(got[0] - base[0]), kernel_delta=abs(got[1] - base[1]))


def test_cka_more_pairs_than_one_launch_sequence():
    """pairs = 8195 > the 8192 pairs of one launch sequence: the second chunk's input and output offsets and the scratch it reuses.
    Five distinct 4 x 2 pairs repeated cyclically; row k must be row k mod 5 of the 5-pair call bit for bit.  The C ABI directly, the
    scratch exactly mi_cka_scratch_bytes(8195, 4, 2) with a guard behind it."""
    from exploring_meta_amd import _lib
    lib = _lib.load()
    pairs, n, p = 8195, 4, 2
    cases = [('gauss', 90), ('relu', 91), ('gauss', 92), ('relu', 93), ('gauss', 94)]
    mats = [O.make_case(kind, seed, n, p) for kind, seed in cases]
    x5 = torch.from_numpy(np.stack([m[0] for m in mats])).cuda()
    y5 = torch.from_numpy(np.stack([m[1] for m in mats])).cuda()
    small = torch.stack(list(_cka(x5, y5)), dim=1)                                   # [5, 4]
    worst = [0.0, 0.0]
    for k, (kind, seed) in enumerate(cases):
        e = _check_nan_aware(small[k].cpu().numpy(), _oracle_row(kind, seed, n, p, 0.0))
        worst = [max(a, b) for a, b in zip(worst, e)]
    idx = torch.arange(pairs, device='cuda') % 5
    xs, ys = x5[idx].contiguous(), y5[idx].contiguous()
    need = lib.mi_cka_scratch_bytes(pairs, n, p)
    assert 0 < need == lib.mi_cka_scratch_bytes(8192, n, p)
    guard = 4096
    scratch = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device='cuda')
    out = torch.full((pairs + 1, 4), -7.0, dtype=torch.float64, device='cuda')
    _lib.check(lib.mi_cka(torch.cuda.current_stream().cuda_stream, xs.data_ptr(), ys.data_ptr(), pairs, n, p, 0.0, scratch.data_ptr(), need,
                          out.data_ptr()))
    torch.cuda.synchronize()
    assert bool((scratch[need:] == 0xA5).all()) and bool((out[pairs] == -7.0).all())
    same = out[:pairs].view(torch.int64) == small[idx].contiguous().view(torch.int64)
    bad = (~same.all(dim=1)).nonzero().flatten().tolist()
    assert not bad, ('first rows that differ from the 5-pair call', bad[:8])
    report('cka_8195_pairs', oracle_cka=worst[0], oracle_sigma2=worst[1], rows_differing=len(bad))
