"""The TRPO entry points against the outputs of the commit before the one-step and the K-step implementations became one
(tests/trpo_parity_cases.py; the fixture holds the inputs and that build's outputs, recorded by tools/record_trpo_parity.py).

Where the earlier build ran the kernels this one runs, with the same arguments at other addresses -- the fused sweeps at K = 1, the
K-step path at K = 2 -- the outputs are bit-identical.  Where K = 1 used to run the one-step per-layer drivers (gauss_kernel) and now
runs the K-step ones (gauss2_kernel; the same formulas, its f'' term a zero added), vectors agree to 1e-6 relative: the bar of the
test this one replaces, which held the two routes to each other on the tanh general case."""
import numpy as np
import pytest
import torch

import trpo_parity_cases as TP
from gpu_utils import rel_err, report

pytestmark = pytest.mark.gpu


def _s(a):
    return float(np.asarray(a).reshape(-1)[0])


@pytest.fixture(scope='module')
def parent():
    return np.load(TP.FIXTURE)


def _scalar_bars(case, want):
    """name -> allowed |difference| between two routes (the bars test_fused_fvp_sweeps_... uses between its two routes)."""
    loss, kl = abs(_s(want['loss'])), _s(want['kl'])
    bars = dict(loss=1e-6 * max(1.0, loss), kl=1e-6 * max(kl, 1e-3) if TP.general_case(case) else 1e-7)
    if 'cand_loss' in want:
        bars.update(cand_loss=2e-6 * max(1.0, abs(_s(want['cand_loss']))), cand_kl=1e-6 * max(_s(want['cand_kl']), 1e-3))
    return bars


@pytest.mark.parametrize('case', list(TP.CASES))
def test_trpo_entry_points_reproduce_the_commit_before_their_unification(case, parent):
    name, _, bar, fn, kw = TP.CASES[case]
    want = TP.expected(parent, case)
    got = fn(TP.engine(name), TP.load_inputs(parent, name), **kw)
    assert sorted(got) == sorted(want)
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    equal = {k: bool(np.array_equal(got[k], want[k])) for k in want}
    diff = {k: (abs(_s(got[k]) - _s(want[k])) if k in TP.SCALARS else rel_err(got[k], want[k])) for k in want}
    report(f'trpo_parity[{case}]', bar=bar, bit_identical=equal, diff=diff)
    if bar == 'bitwise':
        assert all(equal.values()), equal
        return
    bars = _scalar_bars(case, want)
    for k in want:
        assert diff[k] <= bars[k] if k in TP.SCALARS else diff[k] < 1e-6, (k, diff[k])


def test_trpo_methods_refuse_arrays_that_do_not_fit_k_t_b(parent):
    """The library sizes every read from (K, T, B) = sup['states'].shape[:3]: a support replay passed the old way, without its leading
    [K] axis, would make T of B and B of S and read the query arrays far out of bounds.  PolicyEngine refuses it, and any other array
    that does not fit, before a launch."""
    x, eng = TP.load_inputs(parent, 'odd'), TP.engine('odd')
    flat = {k: v[0] for k, v in x.sup.items()}
    with pytest.raises(ValueError, match='leading'):
        eng.surrogate(x.theta, flat, x.qry, x.old_loc, x.old_scale, x.lr, True)
    for call in (lambda: eng.fvp(flat, x.qry, x.lr, TP.DAMPING, x.v[0]),
                 lambda: eng.kl_prepare(flat, x.qry, x.old_loc, x.old_scale, x.lr),
                 lambda: eng.fvp_general(flat, x.qry, x.old_scale, x.lr, TP.DAMPING, x.v[0]),
                 lambda: eng.surrogate(x.theta, x.sup, x.qry, x.old_loc[:, :-1], x.old_scale, x.lr, False),
                 lambda: eng.surrogate(x.theta, x.sup, dict(x.qry, count=x.qry['count'][:-1]), x.old_loc, x.old_scale, x.lr, False),
                 lambda: eng.fvp(x.sup, x.qry, x.lr, TP.DAMPING, x.v[0][:-1])):
        with pytest.raises(ValueError):
            call()
    loss, kl, _ = eng.surrogate(x.theta, x.sup, x.qry, x.old_loc, x.old_scale, x.lr, False)      # the engine is unharmed
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(kl).all())
