"""The task-by-task walk (fast_adapt_vpg / fast_adapt_ppo / fast_adapt_trpo, single_ppo_update, trpo_update -> trpo_a2c_loss) against
what the commit before it became the one-task case of the batched adapt loop computed (tests/golden/adapt_walk_parent.npz, recorded
by tools/record_adapt_walk_parity.py from that commit's package; the calls: tests/adapt_walk_parity_cases.py).

Expected bit for bit: the adapted parameters (recorded as SHA-256 digests of their bytes: in full they would take the fixture past
the size a committed file may have), the row counts of every run and the baseline weights.  theta_k from chained
mi_policy_update calls runs the launches of the replay inside mi_policy_meta_batch in the same order; what differs from the earlier
walk is the padded length of the meta_batch call alone, padding rows enter as zeros and the reductions have a fixed tree.  The row
counts equal to the earlier commit's, with the parameters of every run equal, mean replays equal to the earlier commit's: a rollout
is a pure function of (parameters, goal, seed, id), so the replays are not stored.  The other quantities are held to the bars between
walk and batched call of tests/test_gpu_adapt_tasks.py (valid_loss rtol 1e-5, reward 1e-6 relative, gradient rel_err <= 1e-5, success
equal) and reported as bit-identical or not."""
import numpy as np
import pytest

import adapt_walk_parity_cases as WP
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import rl as RLM
from gpu_utils import rel_err, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def parent():
    return np.load(WP.FIXTURE)


@pytest.mark.parametrize('call', list(WP.CALLS))
def test_the_walk_computes_what_the_earlier_commit_computed(call, parent, monkeypatch):
    fn, arg, host = WP.CALLS[call]
    if host:
        monkeypatch.setattr(RLM, '_gae_on_device', lambda *a: False)
    got = {k: np.asarray(v) for k, v in fn(cf, arg).items()}
    want = {k: parent[f'{call}/{k}'] for k in got}
    same = {k: bool(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes()) for k in got}
    report(f'adapt_walk_parity[{call}]', **{f'bit_identical_{k}': v for k, v in same.items()},
           **{f'rel_{k}': rel_err(got[k], want[k]) for k in got if not same[k] and got[k].dtype.kind == 'f'})
    for k in got:
        assert got[k].shape == want[k].shape, k
        if k.endswith(('theta_sha256', 'counts', 'baseline', 'success')):
            assert same[k], k
        elif k.endswith('valid_loss'):
            np.testing.assert_allclose(got[k], want[k], rtol=1e-5, atol=0, err_msg=k)
        elif k == 'reward':
            assert (np.abs(got[k] - want[k]) <= 1e-6 * np.abs(want[k])).all(), k
        else:
            assert k == 'grad' and rel_err(got[k], want[k]) <= 1e-5, k
