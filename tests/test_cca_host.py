"""CCA without a GPU: the fp64 restatement (tests/cca_oracle.py) against the reference's own results (golden_cca.npz), the C ABI's
declarations, argument checks and scratch size (include/mi_maml.h, mi_cca), and the degenerate rules of the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import cca_oracle as O
from exploring_meta_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'golden_cca.npz'), allow_pickle=False)


def test_golden_lists_the_oracle_cases(golden):
    assert [(str(k), int(s), int(n), int(p), float(e)) for k, s, n, p, e in
            zip(golden['kind'], golden['seed'], golden['n'], golden['p'], golden['epsilon'])] == [tuple(c) for c in O.CASES]
    assert float(golden['threshold']) == O.THRESHOLD
    kinds = {c[0] for c in O.CASES}
    assert {'gauss', 'relu', 'rep', 'same', 'rot', 'dead', 'dupcol', 'lindep'} <= kinds
    assert any(c[3] % 2 == 1 and c[3] != 25 and c[3] > 1 for c in O.CASES) and any(c[3] == 64 for c in O.CASES)


@pytest.mark.parametrize('idx', range(len(O.CASES)))
def test_oracle_reproduces_reference(golden, idx):
    kind, seed, n, p, eps = O.CASES[idx]
    x, y = O.make_case(kind, seed, n, p)
    r = O.cca(x, y, eps, O.THRESHOLD)
    mean, tmean, total, cond_x, cond_y = golden['stats'][idx]
    bar = O.bar(cond_x, cond_y)
    want = golden['coefs'][idx]
    want = want[~np.isnan(want)]
    assert r['count'] == len(want) == len(r['coefs'])
    err = max(np.abs(r['coefs'] - want).max(), abs(r['mean'] - mean), abs(r['thresholded_mean'] - tmean), abs(r['sum'] - total))
    assert err <= bar, (err, bar)
    assert np.array_equal(r['x_idxs'], golden['x_idxs'][idx, :p]) and np.array_equal(r['y_idxs'], golden['y_idxs'][idx, :p])
    assert r['cond_x'] == cond_x and r['cond_y'] == cond_y
    # the threshold index does not hinge on rounding
    assert np.abs(O.partial_ratios(want) - O.THRESHOLD).min() > 1e-6


def test_golden_special_cases(golden):
    for idx, (kind, seed, n, p, eps) in enumerate(O.CASES):
        kx, ky = int(golden['x_idxs'][idx].sum()), int(golden['y_idxs'][idx].sum())
        cond = max(golden['stats'][idx, 3:5])
        if kind == 'dead':
            assert (kx, ky) == (24, 23) and int((~np.isnan(golden['coefs'][idx])).sum()) == 23
        else:
            assert (kx, ky) == (p, p)
        if kind in ('dupcol', 'lindep') and eps == 1e-10:
            assert 1e10 < cond < 3e10
        if kind in ('same', 'rot'):
            assert abs(golden['stats'][idx, 0] - 1.0) <= 10 * max(eps, 1e-15)


def test_oracle_degenerate_rules():
    z = O.make_case('gauss', 23, 50, 4)[0]
    ones = np.ones((50, 4), np.float32)
    for eps in (0.0, 1e-10):
        for a, b in ((ones, z), (z, ones), (ones, ones)):
            r = O.cca(a, b, eps)
            assert r['mean'] == r['thresholded_mean'] == r['sum'] == 0.0 and r['count'] == 0 and len(r['coefs']) == 0
    # epsilon = 0 with dead columns: finite; the leading coefficients and the sum are those of the matrices with the columns
    # deleted, a cut direction adds a zero coefficient (count stays p)
    x, y = O.make_case('dead', 9, 800, 25)
    r = O.cca(x, y, 0.0)
    d = O.cca(np.delete(x, O.DEAD_X, axis=1), np.delete(y, O.DEAD_Y, axis=1), 0.0)
    assert r['count'] == 25 and d['count'] == 23 and np.isinf(r['cond_x']) and np.isinf(r['cond_y'])
    assert np.all(np.isfinite(r['coefs']))
    assert np.abs(r['coefs'][:23] - d['coefs']).max() <= 1e-9 and abs(r['sum'] - d['sum']) <= 1e-9
    assert np.abs(r['coefs'][23:]).max() <= 1e-9


def test_header_declares_and_lib_binds_cca():
    header = open(os.path.join(REPO, 'include', 'mi_maml.h')).read()
    assert 'size_t mi_cca_scratch_bytes(int pairs, int n, int p);' in header
    assert 'int mi_cca(void* stream, const float* x, const float* y, int pairs, int n, int p, double epsilon, double threshold,' in header
    assert 'mi_cca' in _lib.EXPORTS and 'mi_cca_scratch_bytes' in _lib.EXPORTS


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libmi_maml.so is not built (run __graft_entry__.build())')
    return _lib.load()


def _ptr():
    buf = C.create_string_buffer(64)
    return buf, C.cast(buf, C.c_void_p)


@pytest.mark.parametrize('pairs,n,p', [(1, 100, 0), (1, 100, 65), (1, 1, 5), (0, 100, 5), (1, (1 << 18) + 1, 5)])
def test_abi_rejects_bad_shapes(lib, pairs, n, p):
    buf, ptr = _ptr()
    assert lib.mi_cca_scratch_bytes(pairs, n, p) == 0
    assert lib.mi_cca(None, ptr, ptr, pairs, n, p, 0.0, 0.98, ptr, 1 << 40, ptr, ptr) == -1      # MI_ERR_ARG, before any HIP call
    assert b'mi_cca' in lib.mi_last_error(None)


@pytest.mark.parametrize('eps,thr', [(-1e-12, 0.98), (float('nan'), 0.98), (0.0, -0.1), (0.0, 1.5), (0.0, float('nan'))])
def test_abi_rejects_bad_epsilon_and_threshold(lib, eps, thr):
    buf, ptr = _ptr()
    assert lib.mi_cca(None, ptr, ptr, 2, 100, 5, eps, thr, ptr, 1 << 40, ptr, ptr) == -1
    assert b'mi_cca' in lib.mi_last_error(None)


def test_abi_rejects_null_pointers_and_small_scratch(lib):
    buf, ptr = _ptr()
    for k in range(5):
        a = [ptr] * 5
        a[k] = None
        x, y, s, c, st = a
        assert lib.mi_cca(None, x, y, 2, 100, 5, 0.0, 0.98, s, 1 << 40, c, st) == -1
    need = lib.mi_cca_scratch_bytes(3, 1000, 25)
    assert need > 0
    assert lib.mi_cca(None, ptr, ptr, 3, 1000, 25, 0.0, 0.98, ptr, need - 1, ptr, ptr) == -3       # MI_ERR_WORKSPACE


def test_scratch_holds_no_n_sized_temporary(lib):
    a, b = lib.mi_cca_scratch_bytes(10, 1 << 17, 25), lib.mi_cca_scratch_bytes(10, 1 << 18, 25)
    assert 0 < a == b                                         # the row chunks are capped at 64: nothing grows with n past that
    assert lib.mi_cca_scratch_bytes(10, 56448, 25) <= a < 10 * 2 * 56448 * 25 * 4        # less than the layer-1 inputs themselves


def test_cca_has_no_cpu_fallback():
    """CPU tensors are refused by the batched call; without a GPU the reference-named function raises too."""
    import torch
    from exploring_meta_amd.utils.cca import cca, get_cca_similarity
    x = O.make_case('gauss', 1, 10, 3)[0]
    with pytest.raises(RuntimeError):
        cca(torch.from_numpy(x), torch.from_numpy(x))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            get_cca_similarity(x.T, x.T)
    with pytest.raises(NotImplementedError, match='coef_x'):
        get_cca_similarity(x.T, x.T, compute_dirns=True)
    with pytest.raises(AssertionError):
        get_cca_similarity(x, x)                              # neurons >= datapoints
    with pytest.raises(AssertionError):
        get_cca_similarity(x.T, x.T[:, :9])


# ---- the inputs of the limit tests (tests/test_gpu_cca.py), checked without a GPU

def test_limit_cases_cover_the_stated_edges_and_stay_out_of_the_golden_table():
    shapes = [(n, p, eps, len(zx), len(zy)) for _, _, n, p, eps, zx, zy in O.LIMIT_CASES]
    assert shapes == [(300, 63, 1e-10, 0, 0), (300, 64, 1e-10, 1, 3), (200, 3, 1e-10, 1, 0), (200, 3, 1e-10, 0, 1), (50, 1, 1e-10, 0, 0),
                      (50, 2, 0.0, 0, 0), (5, 25, 1e-6, 0, 0), (1025, 3, 1e-10, 0, 0), (70001, 3, 1e-10, 0, 0), (1 << 18, 2, 1e-10, 0, 0)]
    assert O.LIMIT_CASES[1][5:] == ((3,), (7, 8, 9))
    assert not {c[:5] for c in O.LIMIT_CASES} & set(O.CASES)
    assert sum(n >= 4000 for n, *_ in shapes) == 2                       # the two linear-cost oracle calls
    assert (70001 + 1023) // 1024 > 64 >= (65536 + 1023) // 1024        # the row-chunk cap binds from n = 65537 on


@pytest.mark.parametrize('idx', range(8))                                 # (the two large cases run once, beside the GPU)
def test_limit_cases_keep_what_they_are_meant_to_keep(idx):
    kind, seed, n, p, eps, zx, zy = O.LIMIT_CASES[idx]
    x, y = O.make_limit_case(kind, seed, n, p, zx, zy)
    r = O.cca(x, y, eps, O.THRESHOLD)
    assert (r['kept_x'], r['kept_y'], r['count']) == (p - len(zx), p - len(zy), p - max(len(zx), len(zy)))
    assert not r['x_idxs'][list(zx)].any() and not r['y_idxs'][list(zy)].any()
    assert np.all(np.isfinite(r['coefs'])) and np.isfinite(r['cond_x']) and np.isfinite(r['cond_y'])
    if n < p:
        assert 1e6 < max(r['cond_x'], r['cond_y']) < 1e7 and O.bar(r['cond_x'], r['cond_y']) < 1e-6
    else:
        assert O.bar(r['cond_x'], r['cond_y']) == 1e-9


def test_threshold_ends_of_the_restated_sum_threshold():
    x, y = O.make_case('relu', 9, 800, 25)
    s = O.cca(x, y, 1e-10)['coefs']
    idx0, mean0 = O.thresholded(s, 0.0)
    idx1, mean1 = O.thresholded(s, 1.0)
    assert idx0 == 0 and np.isnan(mean0) and idx1 == 25 and mean1 == float(s.mean()) and s.min() > 1e-4


def test_the_seven_pairs_of_the_many_pairs_call_differ_and_include_degenerate_ones():
    kept = []
    for kind, seed in O.PAIR_CASES:
        x, y = O.make_case(kind, seed, 3, 2)
        r = O.cca(x, y, 1e-6)
        kept.append((r['kept_x'], r['kept_y']))
    assert len(O.PAIR_CASES) == 7 and (1, 0) in kept and (2, 1) in kept and kept.count((2, 2)) == 5


def test_scratch_of_many_pairs(lib):
    assert lib.mi_cca_scratch_bytes(70000, 3, 2) >= 70000 * (16 + 16 + 2 * 2 * 8 + 3 * 4 * 8)
    assert lib.mi_cca_scratch_bytes(1 << 20, 3, 2) > 0 == lib.mi_cca_scratch_bytes((1 << 20) + 1, 3, 2)
