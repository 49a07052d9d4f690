"""Record tests/golden/policy_call_parent.npz: what every PolicyEngine call that takes an inner-loop step (meta_batch / meta_batch_lr, update,
adapt, the TRPO calls), in its scalar and in its table form, and the workspace-size queries computed on the commit BEFORE the policy side
got one step descriptor per layer, for the cases of tests/policy_call_parity_cases.py.

The fixture judges that change, so it is recorded with the earlier commit's package AND library, never with the code under test:

    git worktree add /tmp/before <commit> && make -C /tmp/before/exploring_meta_amd/csrc -j16
    PYTHONPATH=/tmp/before python tools/record_policy_call_parity.py [out.npz [prefix]]

With a prefix only the cases whose names start with it are run, and the other arrays of an existing out.npz are kept.  Needs the GPU."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [REPO, os.path.join(REPO, 'tests')]                # behind PYTHONPATH: the earlier commit's package is found first


def main():
    import exploring_meta_amd
    from exploring_meta_amd import _lib
    from exploring_meta_amd.engine import PolicyEngine
    where = os.path.dirname(os.path.abspath(exploring_meta_amd.__file__))
    if where == os.path.join(REPO, 'exploring_meta_amd') or 'MI_MAML_LIB' in os.environ:
        sys.exit('this is the package (or a chosen library) under test: put a built worktree of the earlier commit on PYTHONPATH')
    if hasattr(PolicyEngine, '_step_args'):
        sys.exit(f'{where} is not the earlier commit: its PolicyEngine already describes the step once')
    import policy_call_parity_cases as PP
    out = sys.argv[1] if len(sys.argv) > 1 else PP.FIXTURE
    only = sys.argv[2] if len(sys.argv) > 2 else ''
    arrays = dict(np.load(out)) if only and os.path.exists(out) else {}
    arrays.update(PP.compute(only))
    np.savez_compressed(out, **arrays)
    print(f'{len(arrays)} cases, {sum(a.size for a in arrays.values())} lines -> {out}: {os.path.getsize(out)} bytes '
          f'(package: {where}, library: {_lib.LIB_PATH})')


if __name__ == '__main__':
    main()
