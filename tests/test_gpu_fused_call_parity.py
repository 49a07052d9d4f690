"""The fused MAML / ANIL calls, the step-wise learner, graph mode, the autograd layer and the workspace sizes against what the commit
before the call descriptor (one description of a fused call per layer: the MetaCall struct, MetaEngine._maml_call, one autograd
Function) computed: tests/golden/fused_call_parent.npz, recorded by tools/record_fused_call_parity.py from that commit's package and
library; the calls: tests/fused_call_parity_cases.py.

That change moved host code only, the arithmetic has a fixed order and graph replay is held bitwise to eager, so every quantity is
expected bit for bit: losses, accuracies, step-size gradients of per-tensor steps and sizes as they are, gradients and logits as SHA-256
digests of their bytes, and so is the whole workspace after a call that found it zeroed (layout/*: every intermediate at the offset the
earlier plans gave it, which no entry point reports in full).  Checked to fail: with lr_vec left out of the graph key graph/maml_lr fails,
with two takes of the shared partial-buffer function swapped layout/* fail.  Graph mode's eager, capture and replay calls are held to the fixture of the eager call, the deferred outer
backward to the fixture of the undeferred run (fused_call_parity_cases.fixture_key)."""
import numpy as np
import pytest

import fused_call_parity_cases as FP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def parent():
    return np.load(FP.FIXTURE)


@pytest.mark.parametrize('call', list(FP.CALLS))
def test_the_call_computes_what_the_earlier_commit_computed(call, parent):
    fn, kw = FP.CALLS[call]
    got = fn(**kw)
    recorded = {k.split(call + '/', 1)[1] for k in parent.files if k.startswith(call + '/')}
    assert set(got) == recorded, sorted(set(got) ^ recorded)
    for k, v in got.items():
        want = parent[FP.fixture_key(call, k)]
        print(f'fused_call_parity[{call}] {k}: {"bit-identical" if v.tobytes() == want.tobytes() else (v, want)}')
        assert v.shape == want.shape and v.dtype == want.dtype and v.tobytes() == want.tobytes(), (call, k)
