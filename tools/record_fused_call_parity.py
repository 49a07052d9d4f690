"""Record tests/golden/fused_call_parent.npz: what the fused MAML / ANIL calls, the step-wise learner, graph mode, the autograd layer and
the workspace-size queries computed on the commit BEFORE a fused call got one description per layer, for the calls of
tests/fused_call_parity_cases.py.

The fixture judges that change, so it is recorded with the earlier commit's package AND library, never with the code under test:

    git worktree add /tmp/before <commit> && make -C /tmp/before/exploring_meta_amd/csrc -j16
    PYTHONPATH=/tmp/before python tools/record_fused_call_parity.py [out.npz [prefix]]

With a prefix only the calls whose names start with it are run, and the other arrays of an existing out.npz are kept.

Every quantity is stored under its own name; where the test expects one call to give what another gave (graph mode against eager, the
deferred outer backward against the undeferred run) the recorder checks that the earlier commit does.  Needs the GPU."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [REPO, os.path.join(REPO, 'tests')]                # behind PYTHONPATH: the earlier commit's package is found first


def main():
    import exploring_meta_amd
    from exploring_meta_amd import _lib
    from exploring_meta_amd.core_functions import vision
    where = os.path.dirname(os.path.abspath(exploring_meta_amd.__file__))
    if where == os.path.join(REPO, 'exploring_meta_amd') or 'MI_MAML_LIB' in os.environ:
        sys.exit('this is the package (or a chosen library) under test: put a built worktree of the earlier commit on PYTHONPATH')
    if not hasattr(vision, '_FusedFastAdaptLR'):
        sys.exit(f'{where} is not the earlier commit: its vector call is already a case of the one autograd Function')
    import fused_call_parity_cases as FP
    out = sys.argv[1] if len(sys.argv) > 1 else FP.FIXTURE
    only = sys.argv[2] if len(sys.argv) > 2 else ''
    arrays = dict(np.load(out)) if only and os.path.exists(out) else {}
    arrays.update(FP.compute(only))
    assert all(np.isfinite(a).all() for a in arrays.values() if a.dtype.kind == 'f')
    differ = [name for call in FP.CALLS for name in arrays if name.startswith(call + '/')
              and arrays[name].tobytes() != arrays[FP.fixture_key(call, name[len(call) + 1:])].tobytes()]
    np.savez_compressed(out, **arrays)
    print(f'{len(arrays)} arrays -> {out}: {os.path.getsize(out)} bytes (package: {where}, library: {_lib.LIB_PATH})')
    if differ:
        sys.exit(f'the earlier commit itself does not give the same bits where the test expects them: {differ}')


if __name__ == '__main__':
    main()
