"""Record tests/golden/adapt_walk_parent.npz: what the task-by-task walk (fast_adapt_vpg / fast_adapt_ppo / fast_adapt_trpo,
single_ppo_update, trpo_update -> trpo_a2c_loss) computed on the commit BEFORE it became the one-task case of the batched adapt loop,
for the calls of tests/adapt_walk_parity_cases.py.

The fixture judges that change, so it is recorded with the earlier commit's Python package, never with the code under test.  The
library did not change, so the in-tree build serves:

    git worktree add /tmp/before <commit>
    PYTHONPATH=/tmp/before MI_MAML_LIB=$PWD/exploring_meta_amd/csrc/libmi_maml.so python tools/record_adapt_walk_parity.py [out.npz]

Needs the GPU."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [REPO, os.path.join(REPO, 'tests')]                # behind PYTHONPATH: the earlier commit's package is found first


def main():
    import exploring_meta_amd
    from exploring_meta_amd import core_functions as cf
    from exploring_meta_amd.core_functions import rl
    where = os.path.dirname(os.path.abspath(exploring_meta_amd.__file__))
    if where == os.path.join(REPO, 'exploring_meta_amd'):
        sys.exit('this is the package under test: put a worktree of the earlier commit on PYTHONPATH')
    if not hasattr(rl, '_replay_meta'):
        sys.exit(f'{where} is not the earlier commit: its walk already runs the batched adapt loop')
    import adapt_walk_parity_cases as WP
    out = sys.argv[1] if len(sys.argv) > 1 else WP.FIXTURE
    arrays = WP.compute(cf, rl)
    assert all(np.isfinite(a).all() for a in arrays.values() if a.dtype.kind == 'f')
    np.savez_compressed(out, **arrays)
    print(f'{len(arrays)} arrays -> {out}: {os.path.getsize(out)} bytes (package: {where})')


if __name__ == '__main__':
    main()
