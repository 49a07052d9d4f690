"""What the case table of tests/conv_shape_cases.py covers, proved on the CPU from the launchers' own decisions: mi_debug_wgrad_plan and
mi_debug_conv_plan return the plan launch_wgrad3x3 / launch_conv3x3 launch from (host arithmetic, no GPU).  For every operand form of
conftest.CONV_FORMS and for one and two terms the union of plans over the table must hold every item of the coverage list below; the same
query applied to the tables the kernel tests had before (CONV_CASES, TAN_CONV_CASES, BIG_CONV) is printed for comparison."""
import pytest

import conv_shape_cases as CS
from conftest import CONV_FORMS, apply_conv_form
from exploring_meta_amd import _lib

PIECES = (8, 12, 16, 20, 24)


@pytest.fixture(params=list(CONV_FORMS))
def form(request):
    lb = _lib.load()
    restore = apply_conv_form(lb, request.param)
    yield lb, request.param
    restore()


def _wgrad_items(lb, shapes, nterms):
    """shapes: (T, n, h, w, ci, co, stride).  Returns the set of coverage items the weight-gradient launches of these shapes reach."""
    got = set()
    for (T, n, h, w, ci, co, stride) in shapes:
        if ci in (1, 3) and nterms == 2:
            continue                                         # the first layer has no two-term launch
        p = CS.wgrad_plan(lb, T, n, h, w, ci, co, stride, nterms)
        fam = p.family
        got.add(f'{fam}')
        got.add(f'width {w}: {fam}' + (f' c{ci}' if w in (55, 56) else ''))
        if fam == 'rows_f32':
            got.add(f'rows_f32<{p.size}, {"true" if p.exact else "false"}>')
            for tag, on in (('w = 1', w == 1), ('w = 2', w == 2), ('h = 1', h == 1), ('odd h', h % 2 == 1 and h > 1)):
                if on:
                    got.add(f'rows_f32 {tag}')
        elif fam == 'rows_bf16':
            last = p.per_term * nterms - (p.blocks - 1) * p.per_block
            for tag, on in ((f'c{ci}', True), ('w = 16', w == 16), ('partial last unit (w = 17 / 31)', w in (17, 31)), ('h = 1', h == 1),
                            ('workgroup below its 24-unit trip', last < 24)):
                if on:
                    got.add(f'rows_bf16 {tag}')
        elif fam == 'strips_bf16':
            for tag, on in ((f'c{ci}', True), (f'w = {w}', w in (32, 47, 48)), ('w = 42, h != 42', w == 42 and h != 42), ('h < 4', h < 4),
                            ('h % 4 != 0', h % 4 != 0), ('uneven pieces', h > p.size and h % p.size != 0), (f'pieces of {p.size} rows', True),
                            ('at most one item per wave', p.per_block <= 4), ('more than one item per wave', p.per_block > 4),
                            ('fewer items than waves', min(p.per_block, p.per_term * nterms - (p.blocks - 1) * p.per_block) < 4)):
                if on:
                    got.add(f'strips_bf16 {tag}')
        else:
            got.add(f'{fam} chunks of {p.size}')
        if nterms == 2 and fam in ('rows_f32', 'rows_bf16', 'strips_bf16') and CS.straddles_terms(p):
            got.add(f'{fam} workgroup straddles the terms')
    return got


def _wgrad_required(kind, nterms):
    req = {f'rows_f32<{rh}, {e}>' for rh in (4, 5, 7, 8) for e in ('true', 'false')}
    req |= {'rows_f32 w = 1', 'rows_f32 w = 2', 'rows_f32 h = 1', 'rows_f32 odd h', 'chunked chunks of 32', 'chunked chunks of 64'}
    if nterms == 1:
        req |= {'first chunks of 32', 'first chunks of 64'}
    streams = ['rows_f32']
    if kind == 'split':
        streams += ['rows_bf16', 'strips_bf16']
        req |= {'rows_bf16 c32', 'rows_bf16 c64', 'rows_bf16 w = 16', 'rows_bf16 partial last unit (w = 17 / 31)', 'rows_bf16 h = 1',
                'rows_bf16 workgroup below its 24-unit trip'}
        req |= {'strips_bf16 c32', 'strips_bf16 c64', 'strips_bf16 w = 32', 'strips_bf16 w = 48', 'strips_bf16 w = 47',
                'strips_bf16 w = 42, h != 42', 'strips_bf16 h < 4', 'strips_bf16 h % 4 != 0', 'strips_bf16 uneven pieces',
                'strips_bf16 at most one item per wave', 'strips_bf16 more than one item per wave', 'strips_bf16 fewer items than waves'}
        req |= {f'strips_bf16 pieces of {r} rows' for r in PIECES}
        # both sides of every predicate edge
        req |= {'width 15: rows_f32', 'width 16: rows_bf16', 'width 31: rows_bf16', 'width 32: strips_bf16', 'width 41: rows_bf16',
                'width 42: strips_bf16', 'width 55: rows_bf16 c64', 'width 56: strips_bf16 c64'}
    else:
        req |= {f'width {w}: rows_f32' for w in (15, 16, 31, 32, 41, 42)} | {'width 55: rows_f32 c64', 'width 56: rows_f32 c64'}
    if nterms == 2:
        req |= {f'{f} workgroup straddles the terms' for f in streams}
    return req


def _conv_items(lb, shapes, nterms, form_name):
    got = set()
    for (T, n, h, w, ci, co, stride) in shapes:
        launches = [('fwd', CS.EPI_STATS if nterms == 1 else CS.EPI_TSTATS, 0)] + ([('dgrad', CS.EPI_NONE, 1)] if ci >= 32 else [])
        if ci in (1, 3) and nterms == 2:
            continue
        for tag, epi, mode in launches:
            p = CS.conv_plan(lb, T, n, h, w, ci, co, stride, nterms, epi, mode)
            got.add(f'{tag} {p.kernel}')
            assert p.stats64 == CS.expected_stats64(p, epi), (T, n, h, w, ci, p)
            if p.kernel == 's1_bf16_16x16' and epi == CS.EPI_STATS:
                got.add('fwd s1_bf16_16x16 statistics ' + ('fp64 per value (one tile per task)' if p.stats64 else 'fp32 per tile'))
            mpix = n * (h if mode else (h - 1) // stride + 1) * (w if mode else (w - 1) // stride + 1)
            partial = mpix % p.tile_pix != 0
            if p.kernel.startswith('s1') and w not in (42, 21) and partial:
                if p.tiles_per_wave > 1 and h * w <= 400:
                    got.add(f'{tag} small map, more than one tile per wave, partial last tile')
                if p.tiles_per_wave >= 6 and (form_name != 'split_bf16' or p.kernel == 's1_bf16_16x16'):
                    got.add(f'{tag} six tiles per wave, partial last tile')
    return got


def _conv_required(form_name, nterms):
    req = {f'{t} small map, more than one tile per wave, partial last tile' for t in ('fwd', 'dgrad')}
    if form_name == 'split_bf16':                            # the form whose kernel depends on the tile count
        req |= {f'{t} six tiles per wave, partial last tile' for t in ('fwd', 'dgrad')} | {'fwd s1_bf16_32x32', 'fwd s1_bf16_16x16'}
    if nterms == 1 and form_name in ('split_bf16', 'split_bf16_16x16'):      # both sides of the 16x16x32 kernel's statistics edge
        req |= {'fwd s1_bf16_16x16 statistics fp32 per tile'}
        if form_name == 'split_bf16_16x16':
            req |= {'fwd s1_bf16_16x16 statistics fp64 per value (one tile per task)'}
    req |= {'fwd generic', 'dgrad generic'} | ({'fwd first'} if nterms == 1 else set())
    return req


def _shapes(cases):
    return [(c.T, c.n, c.h, c.w, c.ci, c.co, c.stride) for c in cases]


def _old_tables():
    import test_gpu_kernels as K
    import test_gpu_tangent_kernels as TK
    one = [tuple(c[1:8]) for c in K.CONV_CASES] + [tuple(c[1:7]) + (1,) for c in TK.BIG_CONV]
    two = [tuple(c[1:8]) for c in TK.TAN_CONV_CASES]
    return {1: one, 2: two}


@pytest.mark.parametrize('nterms', [1, 2])
def test_case_table_covers_every_launcher_boundary(form, nterms):
    lb, name = form
    kind = CS.form_kind(name)
    new = _wgrad_items(lb, _shapes(CS.CASES), nterms) | _conv_items(lb, _shapes(CS.CASES), nterms, name)
    old_shapes = _old_tables()[nterms]
    old = _wgrad_items(lb, old_shapes, nterms) | _conv_items(lb, old_shapes, nterms, name)
    req = _wgrad_required(kind, nterms) | _conv_required(name, nterms)
    print(f'\n[coverage] form {name}, {nterms} term(s): the old tables reach {len(req & old)} of {len(req)} items, the new table {len(req & new)}')
    for item in sorted(req):
        print(f'[coverage]   {"old" if item in old else "   "} {"new" if item in new else "   "}  {item}')
    assert not (req - new), sorted(req - new)


@pytest.mark.parametrize('nterms', [1, 2])
def test_every_case_takes_the_plan_it_is_in_the_table_for(form, nterms):
    lb, name = form
    for c in CS.CASES:
        if c.ci in (1, 3) and nterms == 2:
            continue
        p = CS.case_wgrad_plan(lb, c, nterms)
        assert (p.family, p.size, p.exact) == c.wgrad[(CS.form_kind(name), nterms)], (c.name, p)


def test_one_strip_item_per_workgroup_is_never_chosen(form):
    """The issue's list asks for strip launches with one item per workgroup.  strips_split_bf16 never chooses that: a workgroup of four
    waves takes ceil(items / 4) steps, so a split into one-item workgroups costs what two-item workgroups cost and needs more rounds --
    the strict comparison keeps the coarser split.  Held here over a grid of launches so that a cost function that starts to choose it
    fails this test and gets a case."""
    lb, name = form
    split = CS.form_kind(name) == 'split'
    for c in (32, 64):
        for T in (1, 2, 8, 32, 96):
            for n in (1, 2, 5, 25):
                for h in (1, 4, 5, 17, 42):
                    for w in (32, 42, 48, 64):
                        for nterms in (1, 2):
                            p = CS.wgrad_plan(lb, T, n, h, w, c, c, 1, nterms)
                            if split:
                                assert p.family == 'strips_bf16' and p.per_block >= 2 * nterms, (T, n, h, w, c, nterms, p)
                            else:                              # the fp32 pipe has no strip kernel: the same launches run its rows kernel
                                assert p.family == 'rows_f32', (T, n, h, w, c, nterms, p)


def test_plan_follows_the_operand_form_and_rejects_what_no_kernel_takes():
    import ctypes as C
    lb = _lib.load()
    out = (C.c_int * 8)()
    for name, fam in (('fp32_pipe', 'rows_f32'), ('split_bf16', 'strips_bf16'), ('split_f16', 'strips_bf16')):
        restore = apply_conv_form(lb, name)
        try:
            p = CS.wgrad_plan(lb, 32, 25, 42, 42, 32, 32, 1, 1)
            assert p.family == fam and p.form == CONV_FORMS[name][0]
            if fam == 'strips_bf16':
                assert p.size == 24                           # the benchmark's block 2
        finally:
            restore()
    assert lb.mi_debug_wgrad_plan(2, 3, 8, 8, 3, 32, 1, 2, out) != 0        # the first layer has no two-term weight gradient
    assert lb.mi_debug_wgrad_plan(2, 3, 8, 8, 32, 48, 1, 1, out) != 0       # filters in tiles of 32
    assert lb.mi_debug_wgrad_plan(2, 3, 8, 8, 32, 32, 1, 1, None) != 0
    # the older query is the new one for a 32-filter one-term forward launch
    assert lb.mi_debug_conv_tiles_per_wave(32, 25, 42, 42, 32) == CS.conv_plan(lb, 32, 25, 42, 42, 32, 32, 1, 1, CS.EPI_STATS, 0).tiles_per_wave
