"""Shapes at which the launchers of the hidden-block convolution and weight-gradient kernels (csrc/conv_mfma.hip launch_conv3x3 /
launch_wgrad3x3, csrc/wgrad_bf16.hip) change kernel, template instance or work split, and the launch plan each one is in the table for.
tests/test_conv_plan_host.py proves on the CPU (mi_debug_wgrad_plan / mi_debug_conv_plan: the launchers' own decisions) that the table
covers every boundary for every operand form; tests/test_gpu_conv_shapes.py runs every case against the fp64 restatement and asserts the
plan again, so that a change to a cost function cannot silently move a case onto another kernel."""
import ctypes as C
from collections import namedtuple

WgradPlan = namedtuple('WgradPlan', 'family size exact per_block blocks per_term form nchunks')
ConvPlan = namedtuple('ConvPlan', 'kernel tiles_per_wave ntiles blocks tile_pix waves form stats64')
FAMILIES = ('first', 'chunked', 'rows_f32', 'rows_bf16', 'strips_bf16')
CONV_KERNELS = ('first', 'generic', 's1_f32', 's1_bf16_32x32', 's1_bf16_16x16', 's1_f16')
EPI_NONE, EPI_STATS, EPI_TSTATS = 0, 1, 2

Case = namedtuple('Case', 'name T n h w ci co stride check why wgrad')

# `wgrad`: the weight-gradient plan the case is there for, as (family, size, exact) per term count, under the split operand forms
# ('split': split_f16, split_bf16*) and on the fp32 pipe ('fp32'); one entry where both term counts / both kinds of form take the same.
# size = RH of the fp32 rows kernel, rows per piece of the strip kernel, pixels per chunk of the chunked kernels, 8 for the bf16 rows kernel.
# Recorded from mi_debug_wgrad_plan; test_gpu_conv_shapes.py and test_conv_plan_host.py hold the library to it.
_R = 'rows_f32'
_B = ('rows_bf16', 8, 0)


def _same(p):
    return {('split', 1): p, ('split', 2): p, ('fp32', 1): p, ('fp32', 2): p}


def _sf(split, fp32):
    return {('split', 1): split, ('split', 2): split, ('fp32', 1): fp32, ('fp32', 2): fp32}


def _strips(p1, p2, fp32):
    return {('split', 1): ('strips_bf16', p1, 0), ('split', 2): ('strips_bf16', p2, 0), ('fp32', 1): fp32, ('fp32', 2): fp32}


CASES = [
    # ---- fp32 rows kernel wgrad3x3_rows_mfma_kernel<RH, EXACT>: maps narrower than 16 take it under every operand form
    Case('r8x_8x8', 2, 3, 8, 8, 32, 32, 1, None, '<8, true>: block 3 of a 4-conv-32 model on 32x32 inputs', _same((_R, 8, 1))),
    Case('r8n_8x8_c64', 2, 2, 8, 8, 64, 64, 1, None, '<8, false>: 64 filters never take EXACT', _same((_R, 8, 0))),
    Case('r4x_4x4', 2, 3, 4, 4, 32, 32, 1, None, '<4, true>: block 4 of the same model, one segment per row', _same((_R, 4, 1))),
    Case('r4x_5x12', 2, 2, 5, 12, 32, 32, 1, None, '<4, true> with three segments (inner segment: both halo columns inside), odd height',
         _same((_R, 4, 1))),
    Case('r4n_4x4_c64', 1, 3, 4, 4, 64, 64, 1, None, '<4, false>', _same((_R, 4, 0))),
    Case('r4n_1x1', 2, 4, 1, 1, 32, 32, 1, None, 'width 1, one row: one segment, both halo columns and both halo rows outside',
         _same((_R, 4, 0))),
    Case('r4n_3x1', 2, 3, 3, 1, 32, 32, 1, None, 'width 1, odd height: the second lane half of the last row pair is outside',
         _same((_R, 4, 0))),
    Case('r4n_1x2', 2, 3, 1, 2, 32, 32, 1, None, 'width 2, one row', _same((_R, 4, 0))),
    Case('r5x_5x10', 2, 3, 5, 10, 32, 32, 1, None, '<5, true> with two segments, odd height', _same((_R, 5, 1))),
    Case('r5x_4x15', 2, 2, 4, 15, 32, 32, 1, None, 'w = 15: the last width below wgrad_bf16_ok (three exact segments of 5)',
         _same((_R, 5, 1))),
    Case('r5n_9x9', 2, 2, 9, 9, 32, 32, 1, None, '<5, false>: last segment one column short', _same((_R, 5, 0))),
    Case('r7x_7x14', 2, 2, 7, 14, 32, 32, 1, None, '<7, true> with two segments, odd height', _same((_R, 7, 1))),
    Case('r7n_6x13', 2, 2, 6, 13, 32, 32, 1, None, '<7, false>', _same((_R, 7, 0))),
    # ---- split-bf16 rows kernel wgrad3x3_rows_bf16_kernel (16 <= w, not strips); the fp32 pipe runs its rows kernel on the same maps
    Case('b16_16x16', 2, 3, 16, 16, 32, 32, 1, None, 'w = 16, the edge of wgrad_bf16_ok: block 2 of a 4-conv-32 model on 32x32 inputs',
         _sf(_B, (_R, 8, 1))),
    Case('b16_1x16', 1, 3, 1, 16, 32, 32, 1, None, 'one row, 6 units: fewer than the 24-unit trip of a workgroup', _sf(_B, (_R, 8, 1))),
    Case('b16_5x16_c64', 2, 2, 5, 16, 64, 64, 1, None, 'w = 16 with 64 filters, odd height', _sf(_B, (_R, 8, 0))),
    Case('b17_3x17', 2, 2, 3, 17, 32, 32, 1, None, 'w = 17: the last 8-column unit holds one column', _sf(_B, (_R, 5, 0))),
    Case('b31_4x31_c64', 2, 2, 4, 31, 64, 64, 1, None, 'w = 31, the last width below the strip kernel; partial last unit; 64 filters',
         _sf(_B, (_R, 8, 0))),
    Case('b41_4x41', 2, 2, 4, 41, 32, 32, 1, None, 'w = 41: 17 % padding of three strips, one too many for the strip kernel',
         _sf(_B, (_R, 7, 0))),
    Case('b55_2x55_c64', 1, 2, 2, 55, 64, 64, 1, None, 'w = 55 with 64 filters: below the strip kernel', _sf(_B, (_R, 5, 0))),
    # ---- split-bf16 strip kernel wgrad3x3_strip_bf16_kernel (w >= 32, at most 15 % padding): widths, heights below / not a multiple of the
    # four-row trip, uneven pieces
    Case('s32_1x32', 2, 3, 1, 32, 32, 32, 1, None, 'w = 32 (no padded column), one row: a 4-row piece with three rows outside',
         _strips(4, 4, (_R, 8, 1))),
    Case('s32_5x32', 2, 2, 5, 32, 32, 32, 1, None, 'h = 5: an 8-row piece, second trip with one row', _strips(8, 8, (_R, 8, 1))),
    Case('s32_32x32', 2, 3, 32, 32, 32, 32, 1, None, 'block 2 of a 4-conv-32 model on 64x64 inputs', _strips(8, 8, (_R, 8, 1))),
    Case('s48_3x48', 2, 2, 3, 48, 32, 32, 1, None, 'w = 48 (three full strips), h = 3', _strips(4, 4, (_R, 8, 1))),
    Case('s47_2x47', 2, 2, 2, 47, 32, 32, 1, None, 'w = 47: one padded column, h = 2', _strips(4, 4, (_R, 8, 0))),
    Case('s42_25x42', 2, 2, 25, 42, 32, 32, 1, None, 'w = 42 at a height other than 42', _strips(8, 8, (_R, 7, 1))),
    Case('s56_2x56_c64', 1, 2, 2, 56, 64, 64, 1, None, 'w = 56 with 64 filters: the first width of the strip kernel above 48',
         _strips(4, 4, (_R, 7, 0))),
    # every piece length strips_split_bf16 can choose, for one and for two terms (the cost function sees tasks x images x terms)
    Case('s42_T24_17x42_c64', 24, 1, 17, 42, 64, 64, 1, [0, 23], 'pieces of 12 rows (one term: 12 + 5) and 20 rows (two terms); 3 items per workgroup of 4 waves',
         _strips(12, 20, (_R, 7, 0))),
    Case('s42_T24_25x42_c64', 24, 1, 25, 42, 64, 64, 1, [0, 23], 'pieces of 16 rows (one term): 25 rows as 16 + 9, uneven', _strips(16, 8, (_R, 7, 0))),
    Case('s42_T24_21x42_c64', 24, 1, 21, 42, 64, 64, 1, [1, 22], 'pieces of 24 rows (two terms) holding 21', _strips(12, 24, (_R, 7, 0))),
    Case('s42_T24_n2_17x42_c64', 24, 2, 17, 42, 64, 64, 1, [2, 23], 'pieces of 20 rows (one term) holding 17', _strips(20, 12, (_R, 7, 0))),
    Case('s42_T24_41x42_c64', 24, 1, 41, 42, 64, 64, 1, [0, 12], 'pieces of 24 rows (one term): 41 rows as 24 + 17', _strips(24, 12, (_R, 7, 0))),
    Case('s42_T3_n8_13x42_c64', 3, 8, 13, 42, 64, 64, 1, None, 'pieces of 16 rows (two terms) holding 13; several items per workgroup',
         _strips(8, 16, (_R, 7, 0))),
    Case('s42_T24_n8_13x42', 24, 8, 13, 42, 32, 32, 1, [0, 23], '32 filters: pieces of 16 rows (one term) holding 13', _strips(16, 8, (_R, 7, 1))),
    Case('s42_T12_n10_17x42', 12, 10, 17, 42, 32, 32, 1, [3, 11], '32 filters: pieces of 12 rows (one term: 12 + 5) and of 20 rows (two terms)',
         _strips(12, 20, (_R, 7, 1))),
    Case('s32_T32_n5_8x32_c64', 32, 5, 8, 32, 64, 64, 1, [0, 31], 'five items per workgroup: a wave with two items beside waves with one',
         _strips(8, 8, (_R, 8, 0))),
    # ---- stride-2 kernels (Omniglot-style blocks): wgrad_chunks() = 32 and 64, first layer and hidden
    Case('g2_first_c3_9x11', 2, 3, 9, 11, 3, 32, 2, None, 'first layer, stride 2, odd rectangle: chunks of 32 pixels, partial last chunk',
         _same(('first', 32, 0))),
    Case('g2_first_c1_T32', 32, 21, 28, 28, 1, 64, 2, [0, 31], 'first layer, stride 2: chunks of 64 pixels', _same(('first', 64, 0))),
    Case('g2_hidden_5x7_c64', 2, 3, 5, 7, 64, 64, 2, None, 'hidden stride-2 block on an odd rectangle: chunks of 32 pixels',
         _same(('chunked', 32, 0))),
    Case('g2_hidden_T32', 32, 21, 28, 28, 32, 32, 2, [0, 31], 'hidden stride-2 block: chunks of 64 pixels', _same(('chunked', 64, 0))),
    # ---- forward / dgrad tile split on maps that are not 42 or 21 wide
    Case('c_tpw2_13x13', 32, 25, 13, 13, 32, 32, 1, [0, 31], 'small map, more than one tile per wave under every form, partial last tile',
         _same((_R, 7, 0))),
    Case('c_tpw6_20x20', 32, 25, 20, 20, 32, 32, 1, [5], 'six tiles of 30 pixels per wave: the switch to the 16x16x32 kernel, partial last tile',
         _sf(_B, (_R, 5, 1))),
]
BY_NAME = {c.name: c for c in CASES}


def form_kind(form_name):
    return 'fp32' if form_name == 'fp32_pipe' else 'split'


def out_hw(c):
    return (c.h - 1) // c.stride + 1, (c.w - 1) // c.stride + 1


def wgrad_plan(lib, T, n, h, w, ci, co, stride, nterms):
    out = (C.c_int * 8)()
    rc = lib.mi_debug_wgrad_plan(T, n, h, w, ci, co, stride, nterms, out)
    assert rc == 0, (rc, list(out))
    return WgradPlan(FAMILIES[out[0]], *list(out)[1:8])


def conv_plan(lib, T, n, h, w, ci, co, stride, nterms, epi, mode):
    out = (C.c_int * 8)()
    rc = lib.mi_debug_conv_plan(T, n, h, w, ci, co, stride, nterms, epi, mode, out)
    assert rc == 0, (rc, list(out))
    return ConvPlan(CONV_KERNELS[out[0]], *list(out)[1:8])


def case_wgrad_plan(lib, c, nterms):
    return wgrad_plan(lib, c.T, c.n, c.h, c.w, c.ci, c.co, c.stride, nterms)


def case_conv_plan(lib, c, nterms, epi, mode):
    return conv_plan(lib, c.T, c.n, c.h, c.w, c.ci, c.co, c.stride, nterms, epi, mode)


def expected_conv_kernel(c, form_name, nterms, plan):
    """The kernel a forward / dgrad launch of case c takes under a form of conftest.CONV_FORMS: first layer and stride-2 / ci != co blocks
    have one kernel each; 32-filter stride-1 blocks (64 filters: one-term launches only) follow the form, and the default form
    ('split_bf16') moves to the 16x16x32 kernel from six tiles per wave."""
    if c.ci in (1, 3):
        return 'first'
    if c.stride != 1 or c.ci != c.co:
        return 'generic'
    if form_name == 'fp32_pipe' or (c.ci == 64 and nterms == 2):
        return 's1_f32'
    return {'split_f16': 's1_f16', 'split_bf16_16x16': 's1_bf16_16x16', 'split_bf16_32x32': 's1_bf16_32x32',
            'split_bf16': 's1_bf16_16x16' if plan.tiles_per_wave >= 6 else 's1_bf16_32x32'}[form_name]


def expected_stats64(plan, epi):
    """The 16x16x32 kernel adds a tile's values to the BatchNorm statistics in fp32 first, except where a task's whole map is one tile:
    those launches take the instance that adds every value in fp64 (csrc/conv_b16.h, S64)."""
    return int(plan.kernel == 's1_bf16_16x16' and epi == EPI_STATS and plan.ntiles == 1)


def straddles_terms(p):
    """Two-term launch of a stream kernel: some workgroup's run of the [term][unit] stream holds the boundary between the terms."""
    return p.per_term % p.per_block != 0
