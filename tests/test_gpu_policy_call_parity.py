"""Every PolicyEngine call that takes an inner-loop step -- meta_batch / meta_batch_lr, update, adapt, surrogate, fvp, kl_prepare, fvp_general,
each in its scalar and in its table form -- and the workspace sizes against what the commit before the step descriptor (PolicyStep and the
call structs of csrc/policy.hip, PolicyEngine._step_args / _meta_call, one step closure in core_functions/rl.py) computed:
tests/golden/policy_call_parent.npz, recorded by tools/record_policy_call_parity.py from that commit's package and library; the cases:
tests/policy_call_parity_cases.py.

That change moved host code only and every reduction has a fixed order, so every quantity is expected bit for bit: losses and sizes as
they are, gradients, theta_out and products as SHA-256 digests, and so is the whole workspace after calls that found it pre-sized and zeroed
(layout/*: every intermediate at the offset the earlier plans gave it).  inputs: the digests of the seeded inputs themselves -- where that
case fails, a generator drifted and the other failures say nothing about the code under test.

Checked to fail (mutations of csrc/policy.hip on a scratch copy, never committed):
- PolicyStep::row(k) returning row 0: every meta/*/rowsK case, trpo/relu_k2/rowsK, layout/meta/table and layout/trpo/table fail (12);
- step_advance's scalar form without its head mask: every meta/*/scalar, update/*/scalar and update_in_place/scalar case fails (16);
- the two takes of lr_plan swapped: layout/meta/table fails, the one layout that holds g and prod (the TRPO calls take nothing from
  lr_plan, the scalar layouts have no such arrays).
"""
import numpy as np
import pytest

import policy_call_parity_cases as PP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def parent():
    return np.load(PP.FIXTURE)


@pytest.mark.parametrize('case', list(PP.CASES))
def test_the_call_computes_what_the_earlier_commit_computed(case, parent):
    fn, kw = PP.CASES[case]
    got = {line.split(' ', 1)[0]: line for line in fn(**kw)}
    want = {line.split(' ', 1)[0]: line for line in (x.decode() for x in parent[case])}
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    differ = [v for v in got if got[v] != want[v]]
    for v in got:
        print(f'policy_call_parity[{case}] {v}: {"bit-identical" if got[v] == want[v] else (got[v], want[v])}')
    assert not differ, (case, differ)
