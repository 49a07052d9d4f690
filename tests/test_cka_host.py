"""CKA without a GPU: the fp64 restatement (tests/cka_oracle.py) against the reference's own results (golden_cka.npz), and the
C ABI's argument checks and scratch size (include/mi_maml.h, mi_cka)."""
import ctypes as C
import os

import numpy as np
import pytest

import cka_oracle as O
from exploring_meta_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(HERE, 'golden', 'golden_cka.npz'), allow_pickle=False)


def test_golden_lists_the_oracle_cases(golden):
    assert [(str(k), int(s), int(n), int(p), float(g)) for k, s, n, p, g in
            zip(golden['kind'], golden['seed'], golden['n'], golden['p'], golden['sigma'])] == [tuple(c) for c in O.CASES]


@pytest.mark.parametrize('idx', range(len(O.CASES)))
def test_oracle_reproduces_reference(golden, idx):
    kind, seed, n, p, sigma = O.CASES[idx]
    x, y = O.make_case(kind, seed, n, p)
    r = O.cka(x, y, sigma if sigma > 0 else None)
    lin, ker, sx, sy = golden['result'][idx]
    assert abs(r['linear'] - lin) <= 1e-6 and abs(r['kernel'] - ker) <= 1e-6
    assert abs(r['sigma_x'] - sx) <= 1e-6 * sx and abs(r['sigma_y'] - sy) <= 1e-6 * sy


def test_oracle_degenerate_cases_are_nan():
    x = np.ones((10, 3), np.float32)
    y = O.make_case('gauss', 1, 10, 3)[1]
    r = O.cka(x, y)
    assert np.isnan(r['linear']) and np.isnan(r['kernel']) and np.isnan(r['sigma_x']) and not np.isnan(r['sigma_y'])


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail('libmi_maml.so is not built (run __graft_entry__.build())')
    return _lib.load()


@pytest.mark.parametrize('pairs,n,p', [(1, 100, 0), (1, 100, 129), (1, 1, 5), (0, 100, 5), (1, (1 << 18) + 1, 5)])
def test_abi_rejects_bad_shapes(lib, pairs, n, p):
    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p)
    assert lib.mi_cka_scratch_bytes(pairs, n, p) == 0
    assert lib.mi_cka(None, ptr, ptr, pairs, n, p, 0.0, ptr, 1 << 40, ptr) == -1          # MI_ERR_ARG, before any HIP call
    assert b'mi_cka' in lib.mi_last_error(None)


def test_abi_rejects_null_pointers(lib):
    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p)
    for args in ((None, ptr, ptr, ptr), (ptr, None, ptr, ptr), (ptr, ptr, None, ptr), (ptr, ptr, ptr, None)):
        x, y, s, o = args
        assert lib.mi_cka(None, x, y, 2, 100, 5, 0.0, s, 1 << 40, o) == -1


def test_abi_rejects_small_scratch(lib):
    buf = C.create_string_buffer(64)
    ptr = C.cast(buf, C.c_void_p)
    need = lib.mi_cka_scratch_bytes(3, 1000, 25)
    assert need > 0
    assert lib.mi_cka(None, ptr, ptr, 3, 1000, 25, 0.0, ptr, need - 1, ptr) == -3           # MI_ERR_WORKSPACE


def test_scratch_grows_linearly_in_n(lib):
    n = 56448
    a, b = lib.mi_cka_scratch_bytes(10, n, 25), lib.mi_cka_scratch_bytes(10, 2 * n, 25)
    assert 0 < a < n * n and 0 < b < (2 * n) ** 2
    assert b <= 2 * a + 4096                                   # no term grows faster than n
    assert lib.mi_cka_scratch_bytes(1, 1 << 18, 128) < (1 << 18) ** 2 // 64


def test_cka_has_no_cpu_fallback():
    """CPU tensors are refused by the batched call; without a GPU the reference-named functions raise too."""
    import torch
    from exploring_meta_amd.utils.cka import cka, get_kernel_CKA, get_linear_CKA
    x = O.make_case('gauss', 1, 10, 3)[0]
    with pytest.raises(RuntimeError):
        cka(torch.from_numpy(x), torch.from_numpy(x))
    if not torch.cuda.is_available():
        for fn in (get_linear_CKA, get_kernel_CKA):
            with pytest.raises(RuntimeError):
                fn(x, x)


# ---- the inputs of the limit tests (tests/test_gpu_cka.py): what the GPU side relies on, checked without a GPU

def test_limit_cases_cover_the_stated_edges_and_stay_out_of_the_golden_table():
    shapes = {(c[2], c[3]) for c in O.LIMIT_CASES}
    assert shapes == set(O.LIMIT_SHAPES) and {c[0] for c in O.LIMIT_CASES} == {'gauss', 'relu'}
    assert {(130, 128), (130, 127), (70, 97), (70, 96), (2, 3), (3, 1), (63, 4), (64, 4), (65, 4), (1025, 3), (2049, 2)} == shapes
    assert 512 * 96 + 16384 == 64 * 1024 < 512 * 97 + 16384              # the histogram kernel's dynamic LDS crosses 64 KiB between them
    assert [((n + 63) // 64, (n + 63) // 64 // 8) for n in (65, 1025, 2049)] == [(2, 0), (17, 2), (33, 4)]    # tiles, column splits (0 -> 1)
    assert [c for c in O.LIMIT_CASES if c[4] > 0] == [('gauss', 50, 130, 128, 2.0), ('relu', 50, 130, 128, 2.0)]
    assert all(c[2] < 4000 for c in O.LIMIT_CASES) and not set(O.LIMIT_CASES) & set(O.CASES)


def test_limit_cases_are_nan_only_where_two_rows_coincide():
    """relu at n = 2 makes both rows of Y equal (no nonzero distance, no variance): NaN there and only there."""
    for kind, seed, n, p, sigma in O.LIMIT_CASES:
        if n > 65:
            continue                                                     # (the large ones are plainly non-degenerate and cost seconds)
        x, y = O.make_case(kind, seed, n, p)
        with np.errstate(invalid='ignore', divide='ignore'):
            r = O.cka(x, y, sigma if sigma > 0 else None)
        nans = [k for k in ('linear', 'kernel', 'sigma_x', 'sigma_y') if np.isnan(r[k])]
        assert nans == (['linear', 'kernel', 'sigma_y'] if (kind, n) == ('relu', 2) else []), (kind, seed, n, p, r)


def test_lattice_inputs_have_tied_medians_and_one_splits_its_middle_ranks():
    split = 0
    for sx, sy, n, dup in O.TIE_CASES:
        for seed in (sx, sy):
            x = O.lattice_rows(seed, n, dup)
            assert x.shape == (n, 2) and x.dtype == np.float32 and set(x.ravel().tolist()) <= {0.0, 1.0, 2.0, 3.0}
            if dup is not None:
                assert np.array_equal(x[dup[0]], x[dup[1]])
            v = O.nonzero_sqdists(x)
            assert np.array_equal(v, np.round(v)) and len(set(v.tolist())) <= 9 and v.size < n * (n - 1) // 2       # ties and duplicates
            count, lo, hi = O.middle_ranks(x)
            assert np.count_nonzero(v == lo) > 20 and np.count_nonzero(v == hi) > 20
            exact = O.exact_median_sigma2(x)
            assert abs(O.median_sigma2(x) - exact) <= 4 * np.finfo(np.float64).eps * exact       # the blocked oracle squares a square root
            if lo != hi:
                assert count % 2 == 0 and (lo, hi, exact) == (4.0, 5.0, 4.5)
                split += 1
    assert split >= 1


def test_scratch_of_a_split_call_is_that_of_its_largest_chunk(lib):
    assert lib.mi_cka_scratch_bytes(8195, 4, 2) == lib.mi_cka_scratch_bytes(8192, 4, 2) > lib.mi_cka_scratch_bytes(5, 4, 2) > 0
