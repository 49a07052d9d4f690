"""Record tests/launch_census.json: the launches per (op name, layer) of every case of tests/test_gpu_launch_census.py.

The table is a reference for the engine's host code, so it is recorded from a build of the commit BEFORE the change it is to judge, never
from the code under test:

    git worktree add /tmp/before <commit> && make -C /tmp/before/exploring_meta_amd/csrc -j16
    MI_MAML_LIB=/tmp/before/exploring_meta_amd/csrc/libmi_maml.so python tools/record_launch_census.py [out.json]

A third argument keeps the rows of an existing table and records only the cases whose names start with it (`... out.json maml_lr`): rows
that judged earlier changes are not re-recorded when cases are added.

Needs the GPU (the counts come from the engine's own per-launch profiling)."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def main():
    import test_gpu_launch_census as census
    out = sys.argv[1] if len(sys.argv) > 1 else census.TABLE
    only = sys.argv[2] if len(sys.argv) > 2 else ''
    table = {}
    if only:
        with open(census.TABLE) as f:
            table = json.load(f)
    table.update((name, census.run_case(case)[0]) for name, case in census.CASES.items() if name.startswith(only))
    with open(out, 'w') as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{len(table)} cases, {sum(map(len, table.values()))} (op, layer) entries -> {out} (library: {os.environ.get("MI_MAML_LIB", "in-tree")})')


if __name__ == '__main__':
    main()
