"""The metric heads on the GPU (mi_metric_head, mi_meta_batch_metric, include/mi_maml.h): the kernel entry against the
fp64 oracle of the definitions (tests/metric_head_oracle.py) at sizes on both sides of every path the kernel takes (feat not a multiple of
4, more than 8 classes, one class, unbalanced classes, ns != nq, the largest ways * feat the header admits and the first it refuses), its
exact edge cases and bitwise relations; the fused call against the oracle on vision_ref's trunk under every operand form; graph replay,
the BatchNorm export, the launch make-up; the Python surface and the drivers.
The edge cases (metric_head_oracle.EDGE_CASES) run what the cases above do not: 64 classes on odd feat > 512 (class lanes 32 to 63, eight
chunks of 8 classes with dfq's read-modify-write over them, the scalar loops past one trip, 37848 of 40960 LDS floats), exactly 8 classes
and 9, nq > 64, nq = 1; a first maximum that sits in the ballot's upper half; 257 tasks against their T = 1 calls; the 16-byte alignment
refusal."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.engine import MetaEngine, ModelSpec
from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from gpu_utils import dev, ptr, rel_err, report, stream
import metric_head_oracle as M
import closed_form_utils as U
from closed_form_utils import census as _census, grads as _grads, held as _held, np_of as _np, same as _same

pytestmark = pytest.mark.gpu

METRICS = (M.PROTO, M.COSINE)
MID = {M.PROTO: 0, M.COSINE: 1}
KERNEL_BAR = 2e-6          # tests/test_gpu_kernels.py's kernel bar
NAMES = ('loss', 'acc', 'logits', 'dfs', 'dfq')


_mspec, _inputs, _trunk = (functools.partial(f, M) for f in (U.mspec, U.inputs, U.trunk))


def _kernel(fs, fq, ys, yq, ways, metric, scale, grad=True, logits=True, fill=None):
    """mi_metric_head on numpy inputs -> (rc, numpy loss, acc, logits, dfs, dfq); outputs the call does not take are None.  fill: the
    outputs start as this value (to see that a refused call leaves them alone)."""
    lib = _lib.load()
    fsd, fqd, ysd, yqd = dev(fs), dev(fq), dev(ys, torch.int32), dev(yq, torch.int32)
    T, ns, feat = fs.shape
    nq = fq.shape[1]
    mk = (lambda *shape: torch.full(shape, float(fill), device='cuda')) if fill is not None else (lambda *shape: torch.empty(*shape, device='cuda'))
    loss, acc = mk(T), mk(T)
    lo = mk(T, nq, ways) if logits else None
    dfs, dfq = (mk(T, ns, feat), mk(T, nq, feat)) if grad else (None, None)
    nscr = lib.mi_metric_head_scratch_bytes(T, ns, nq, feat, ways)
    scr = torch.empty(max(nscr, 1), dtype=torch.uint8, device='cuda')
    rc = lib.mi_metric_head(stream(), ptr(fsd), ptr(fqd), ptr(ysd), ptr(yqd), T, ns, nq, feat, ways, MID[metric], float(scale), ptr(loss),
                            ptr(acc), ptr(lo), ptr(dfs), ptr(dfq), ptr(scr), nscr)
    return (rc,) + _np(loss, acc, lo, dfs, dfq)


def _check_kernel(tag, got, fs, fq, ys, yq, ways, metric, scale):
    """loss, logits, dfs, dfq within max(2e-6, 2 x the fp32 oracle's own error against fp64); accuracy equal."""
    o64 = M.head(fs, fq, ys, yq, ways, metric, scale, torch.float64)
    o32 = M.head(fs, fq, ys, yq, ways, metric, scale, torch.float32)
    errs = {n: rel_err(g, w) for n, g, w in zip(NAMES, got, o64) if n != 'acc'}
    refs = {n: rel_err(r, w) for n, r, w in zip(NAMES, o32, o64) if n != 'acc'}
    report(f'metric_head[{tag}]', **{f'{n}_rel_err': e for n, e in errs.items()}, **{f'ref_fp32_{n}_rel_err': e for n, e in refs.items()})
    for n in errs:
        _held(f'{tag} {n}', errs[n], refs[n], KERNEL_BAR)
    # (one class: no second logit to be close to, every row is clear)
    clear = M.clear_rows(o64[2][None])[0] if ways > 1 else np.ones(o64[2].shape[:2], dtype=bool)
    assert np.array_equal(got[2].argmax(axis=-1)[clear], o64[2].argmax(axis=-1)[clear])
    full = clear.all(axis=-1)
    assert np.array_equal(got[1][full], o64[1][full].astype(np.float32))
    return o64


def _scale_of(metric, feat):
    return (1.0 / feat) if metric == M.PROTO else 4.0      # distances of [0, 3] features grow with feat: keep the logits O(1)


# ---------------------------------------------------------------------------------------------------------------- 1: the kernel entry
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('feat,ways,ns,nq,T', M.KERNEL_CASES + M.EDGE_CASES)
def test_kernel_against_the_fp64_oracle(feat, ways, ns, nq, T, metric):
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, ns, nq, T)
    scale = _scale_of(metric, feat)
    rc, *got = _kernel(fs, fq, ys, yq, ways, metric, scale)
    assert rc == 0, _lib.load().mi_last_error(None)
    o64 = _check_kernel(f'{feat}-{ways}-{ns}/{nq}-T{T}-{metric}', got, fs, fq, ys, yq, ways, metric, scale)
    if ways == 1:       # one class: loss exactly 0, accuracy 1, gradients exactly 0
        assert np.all(got[0] == 0) and np.all(got[1] == 1) and np.all(got[3] == 0) and np.all(got[4] == 0)
    elif feat == 1 and metric == M.COSINE:      # a one-feature row normalises to +-1: its gradient is exactly 0, in the kernel too
        assert np.all(o64[0] > 1e-3) and np.all(o64[3] == 0) and np.all(o64[4] == 0) and np.all(got[3] == 0) and np.all(got[4] == 0)
    else:
        assert np.all(o64[0] > 1e-3) and np.abs(o64[3]).sum() > 0 and np.abs(o64[4]).sum() > 0      # the case tests something


@pytest.mark.parametrize('metric', METRICS)
def test_domain_limit(metric):
    """The largest ways * feat the header admits at 5 ways, ns = nq = 5 (feat 8180: 40955 of 40960 floats of LDS) computes; one feature
    more is MI_ERR_ARG with nothing launched and the outputs untouched."""
    ways, n = 5, 5
    feat = 8180
    assert M.lds_floats(n, n, feat, ways) <= 40960 < M.lds_floats(n, n, feat + 1, ways)
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, n, n, 1)
    scale = _scale_of(metric, feat)
    rc, *got = _kernel(fs, fq, ys, yq, ways, metric, scale)
    assert rc == 0, _lib.load().mi_last_error(None)
    _check_kernel(f'limit-{feat}-{metric}', got, fs, fq, ys, yq, ways, metric, scale)
    fs, fq, ys, yq = M.kernel_inputs(feat + 1, ways, n, n, 1)
    rc, *got = _kernel(fs, fq, ys, yq, ways, metric, scale, fill=-7.0)
    assert rc == -1
    msg = _lib.load().mi_last_error(None).decode()
    assert 'mi_metric_head' in msg and f'feat = {feat + 1}' in msg and 'LDS' in msg, msg
    assert all(np.all(g == -7.0) for g in got)


def test_argument_errors_launch_nothing():
    fs, fq, ys, yq = M.kernel_inputs(32, 5, 5, 5, 1)
    for kw, text in ((dict(ways=65), 'ways'), (dict(scale=0.0), 'scale must be positive'), (dict(scale=-1.0), 'scale must be positive'),
                     (dict(scale=float('nan')), 'scale must be positive')):
        args = dict(ways=5, metric=M.PROTO, scale=1.0)
        args.update(kw)
        rc, *got = _kernel(fs, fq, ys, yq, args['ways'], args['metric'], args['scale'], fill=-7.0)
        assert rc == -1 and text in _lib.load().mi_last_error(None).decode(), _lib.load().mi_last_error(None)
        assert all(np.all(g == -7.0) for g in got)
    lib = _lib.load()
    f, y, out = dev(fs), dev(ys, torch.int32), torch.full((8,), -7.0, device='cuda')
    rc = lib.mi_metric_head(stream(), ptr(f), ptr(f), ptr(y), ptr(y), 1, 5, 5, 32, 5, 2, 1.0, ptr(out), ptr(out[4:]), None, None, None, None, 0)
    assert rc == -1 and 'unknown metric 2' in lib.mi_last_error(None).decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 2: exact edge cases
@pytest.mark.parametrize('metric', METRICS)
def test_all_features_equal_ties_go_to_class_zero(metric):
    ways, n, feat = 5, 10, 40
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, n, n, 1)
    fs[:], fq[:] = 1.5, 1.5
    rc, loss, acc, logits, dfs, dfq = _kernel(fs, fq, ys, yq, ways, metric, 1.0)
    assert rc == 0
    assert np.all(logits == logits[..., :1]), logits                        # every logit of a row ties
    assert acc[0] == np.float32((yq[0] == 0).mean())                        # the first maximum: class 0
    assert loss[0] == pytest.approx(math.log(ways), rel=1e-6)


def test_query_row_equal_to_its_class_vector_has_distance_zero():
    ways, feat = 5, 33
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, ways, ways, 1)             # one shot: the class vector is the support row
    fq[0] = fs[0][yq[0]]
    rc, loss, acc, logits, dfs, dfq = _kernel(fs, fq, ys, yq, ways, M.PROTO, 0.5)
    assert rc == 0
    assert np.all(logits[0][np.arange(ways), yq[0]] == 0) and acc[0] == 1
    off = logits[0][~np.eye(ways, dtype=bool)[yq[0]]]
    assert np.all(off < 0)


def test_cosine_zero_rows_take_the_clamp_branch():
    ways, n, feat = 3, 6, 16
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, n, n, 1)
    fs[0, 1], fq[0, 2] = 0.0, 0.0
    rc, *got = _kernel(fs, fq, ys, yq, ways, M.COSINE, 2.0)
    assert rc == 0 and all(np.isfinite(g).all() for g in got)
    o64 = _check_kernel('cosine-zero-rows', got, fs, fq, ys, yq, ways, M.COSINE, 2.0)
    assert np.all(got[2][0, 2] == 0)                                        # the zero query row: every similarity is 0
    # the clamp branch itself: dx = dxh / 1e-8 on the zero rows, held to the oracle on those rows alone
    assert np.abs(o64[3][0, 1]).max() > 1e6 and np.abs(o64[4][0, 2]).max() > 1e6
    assert rel_err(got[3][0, 1], o64[3][0, 1]) < 1e-5 and rel_err(got[4][0, 2], o64[4][0, 2]) < 1e-5


@pytest.mark.parametrize('feat,ways,n', [(33, 5, 5), (128, 20, 20)])
def test_proto_features_doubled_scale_quartered(feat, ways, n):
    """(2 f, scale / 4): loss, acc and logits bit for bit, dfq and dfs exactly halved."""
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, n, n, 2)
    scale = 1.0 / feat
    rc, *a = _kernel(fs, fq, ys, yq, ways, M.PROTO, scale)
    rc2, *b = _kernel(2 * fs, 2 * fq, ys, yq, ways, M.PROTO, scale / 4)
    assert rc == 0 and rc2 == 0
    _same('doubled', NAMES[:3], b[:3], a[:3])
    assert np.array_equal(b[3], a[3] / 2) and np.array_equal(b[4], a[4] / 2) and np.abs(a[3]).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 3: bitwise relations
@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('feat,ways,ns,nq', [(128, 5, 5, 5), (33, 3, 6, 4), (1600, 5, 25, 25)])
def test_bitwise_relations(feat, ways, ns, nq, metric):
    """Task t of a T = 3 call is the T = 1 call on it; forward-only is the forward half of forward + backward; dfs = dfq = NULL with
    logits given is accepted; logits = NULL with the gradients given too."""
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, ns, nq, 3)
    scale = _scale_of(metric, feat)
    rc, *whole = _kernel(fs, fq, ys, yq, ways, metric, scale)
    assert rc == 0
    for t in range(3):
        rc, *one = _kernel(fs[t:t + 1], fq[t:t + 1], ys[t:t + 1], yq[t:t + 1], ways, metric, scale)
        assert rc == 0
        _same(('task', t), NAMES, [o[0] for o in one], [w[t] for w in whole])
    rc, *fwd = _kernel(fs, fq, ys, yq, ways, metric, scale, grad=False)
    assert rc == 0 and fwd[3] is None and fwd[4] is None
    _same('forward only', NAMES[:3], fwd[:3], whole[:3])
    rc, *nolog = _kernel(fs, fq, ys, yq, ways, metric, scale, logits=False)
    assert rc == 0 and nolog[2] is None
    _same('no logits', ('loss', 'acc', 'dfs', 'dfq'), nolog[:2] + nolog[3:], whole[:2] + whole[3:])


@pytest.mark.parametrize('metric', METRICS)
def test_first_maximum_in_the_upper_lanes(metric):
    """64 classes, one shot, support row 50 a copy of row 40, query rows 0 and 1 that row with labels (40, 50): the logits of classes 40 and
    50 are the row's maximum and bit-equal, the first of them (lane 40, found in the ballot's upper half) is the prediction -- row 0 a hit,
    row 1 a miss; the oracle's argmax takes the first maximum too."""
    ways, feat = 64, 33
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, ways, 2, 1)
    fs[0, 50] = fs[0, 40]
    fq[0, :] = fs[0, 40]
    yq[0] = (40, 50)
    scale = _scale_of(metric, feat)
    rc, loss, acc, logits, dfs, dfq = _kernel(fs, fq, ys, yq, ways, metric, scale)
    assert rc == 0, _lib.load().mi_last_error(None)
    assert np.array_equal(logits[0, :, 40], logits[0, :, 50]) and np.all(logits[0].max(axis=-1) == logits[0, :, 40])
    assert np.all((logits[0] == logits[0, :, 40:41]).sum(axis=-1) == 2)            # (no third class ties)
    assert acc[0] == np.float32(0.5)
    o64 = M.head(fs, fq, ys, yq, ways, metric, scale)
    assert np.array_equal(o64[2][0, :, 40], o64[2][0, :, 50]) and np.array_equal(o64[2][0].argmax(axis=-1), [40, 40]) and o64[1][0] == 0.5
    assert np.array_equal(logits[0].argmax(axis=-1), [40, 40])


@pytest.mark.parametrize('metric', METRICS)
def test_task_independence_beyond_the_cu_count(metric):
    """257 tasks, one more than the 256 CUs: every task of the one launch is the T = 1 call on it, bit for bit."""
    T = 257
    fs, fq, ys, yq = M.kernel_inputs(8, 5, 5, 5, T)
    scale = _scale_of(metric, 8)
    rc, *whole = _kernel(fs, fq, ys, yq, 5, metric, scale)
    assert rc == 0 and all(np.isfinite(w).all() for w in whole) and len({w.tobytes() for w in whole[3]}) == T
    for t in range(T):
        rc, *one = _kernel(fs[t:t + 1], fq[t:t + 1], ys[t:t + 1], yq[t:t + 1], 5, metric, scale)
        assert rc == 0
        _same(('task', t), NAMES, [o[0] for o in one], [w[t] for w in whole])


def test_misaligned_feature_pointers_are_refused():
    """fs, fq, dfs, dfq in turn one float into a larger buffer: MI_ERR_ARG naming the rule, nothing launched, the outputs untouched."""
    lib = _lib.load()
    feat, ways, n = 32, 5, 5
    fs, fq, ys, yq = M.kernel_inputs(feat, ways, n, n, 1)
    ysd, yqd = dev(ys, torch.int32), dev(yq, torch.int32)
    for which in ('fs', 'fq', 'dfs', 'dfq'):
        big = {k: torch.full((n * feat + 8,), -7.0, device='cuda') for k in ('fs', 'fq', 'dfs', 'dfq')}
        v = {k: b[1:1 + n * feat] if k == which else b[4:4 + n * feat] for k, b in big.items()}
        assert all((v[k].data_ptr() % 16 == 0) == (k != which) for k in v)
        v['fs'].copy_(dev(fs).reshape(-1)); v['fq'].copy_(dev(fq).reshape(-1))
        out = torch.full((36,), -7.0, device='cuda')                          # loss at 0, acc at 4, logits (25) at 8
        rc = lib.mi_metric_head(stream(), ptr(v['fs']), ptr(v['fq']), ptr(ysd), ptr(yqd), 1, n, n, feat, ways, MID[M.PROTO], 1.0, ptr(out),
                                ptr(out[4:]), ptr(out[8:]), ptr(v['dfs']), ptr(v['dfq']), None, 0)
        msg = lib.mi_last_error(None).decode()
        assert rc == -1 and 'mi_metric_head' in msg and 'must be 16-byte aligned' in msg, (which, rc, msg)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((big['dfs'] == -7.0).all()) and bool((big['dfq'] == -7.0).all()), which


# ---------------------------------------------------------------------------------------------------------------- 4: the fused call
@functools.lru_cache(maxsize=None)
def _oracle(shape, fp64, ids=None):
    """One oracle run per case and precision (both metrics from one trunk pass), shared by every test that needs it (never modified)."""
    return M.case_oracle(shape, ids, torch.float64 if fp64 else torch.float32)


def _check_fused(tag, shape, metric, got, nf, ids=None):
    loss, acc, grad, logits = got
    o64, o32 = _oracle(shape, True, ids)[metric], _oracle(shape, False, ids)[metric]
    l64 = o64['losses']
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), trunk=rel_err(grad[:nf], o64['grad_feat']))
    refs = dict(loss=np.abs(o32['losses'] - l64) / np.abs(l64), trunk=rel_err(o32['grad_feat'], o64['grad_feat']))
    report(f'metric_fused[{shape}][{metric}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           trunk_rel_err=errs['trunk'], ref_fp32_trunk_rel_err=refs['trunk'])
    _held('loss', errs['loss'], refs['loss'], M.LOSS_FLOOR)
    _held('trunk', errs['trunk'], refs['trunk'], M.GRAD_FLOOR[shape])
    assert grad.shape[0] > nf and np.all(grad[nf:] == 0)                     # the head's entries: exact zeros
    clear = M.clear_rows(o64['logits'][None])[0]
    assert np.all((~clear).sum(axis=-1) * 10 <= clear.shape[-1]), (~clear).sum(axis=-1)
    assert np.array_equal(logits.argmax(axis=-1)[clear], o64['logits'].argmax(axis=-1)[clear])
    full = clear.all(axis=-1)
    assert np.array_equal(acc[full], o64['accs'][full].astype(np.float32))


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('shape', list(M.FUSED_CASES))
def test_fused_call_against_the_fp64_oracle(conv_form, shape, metric):
    """Every operand form: loss within max(1e-4, 2 x the fp32 oracle's error), the trunk gradient within max(the ANIL bar of the same trunk,
    2 x the fp32 oracle's error), argmax equal on clear rows, the head's gradient entries exactly zero (theta's head entries are NaN:
    they are not read).  with_grad = 0: loss, acc and logits bit for bit, meta_grad_out untouched."""
    mspec, theta, data, labels, ways, shots, nf = _inputs(shape, head=float('nan'))
    eng = MetaEngine(mspec)
    scale = M.case_scale(shape, metric)
    got = _np(*eng.meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale, return_logits=True))
    _check_fused(conv_form, shape, metric, got, nf)
    # evaluation only, through the C entry so that meta_grad_out is a buffer of ours
    T, n = data.shape[0], ways * shots
    b = C.c_size_t()
    assert eng.lib.mi_metric_workspace_bytes(eng._h, T, ways, shots, 0, C.byref(b)) == 0
    ws = eng._workspace(b.value)
    out = torch.full((eng.param_count + 2 * T + T * n * ways,), -7.0, device='cuda')
    P = eng.param_count
    rc = eng.lib.mi_meta_batch_metric(eng._h, stream(), ptr(theta), ptr(data), ptr(labels), T, ways, shots, MID[metric], scale, 0, ptr(out[P:]),
                                      ptr(out[P + T:]), ptr(out), ptr(out[P + 2 * T:]), ptr(ws), ws.numel())
    assert rc == 0, eng.lib.mi_last_error(eng._h)
    o = _np(out)[0]
    assert np.all(o[:P] == -7.0)
    _same('with_grad=0', ('loss', 'acc', 'logits'), (o[P:P + T], o[P + T:P + 2 * T], o[P + 2 * T:].reshape(T, n, ways)), (got[0], got[1], got[3]))


@pytest.mark.parametrize('metric', METRICS)
def test_fused_call_single_task(metric):
    """omni at T = 1 (task 0): the oracle's bars, and the bits of task 0 of the four-task call's loss, acc and logits."""
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni', (0,))
    eng = MetaEngine(mspec)
    scale = M.case_scale('omni', metric)
    got = _np(*eng.meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale, return_logits=True))
    _check_fused('T1', 'omni', metric, got, nf, ids=(0,))
    _, _, data4, labels4, _, _, _ = _inputs('omni')
    whole = _np(*eng.meta_batch_metric(theta, data4, labels4, shots, metric=metric, scale=scale, return_logits=True))
    _same('task 0', ('loss', 'acc', 'logits'), (got[0][0], got[1][0], got[3][0]), (whole[0][0], whole[1][0], whole[3][0]))


# ---------------------------------------------------------------------------------------------------------------- 5: engine behaviour
FUSED_NAMES = ('loss', 'acc', 'grad', 'logits')


@pytest.mark.parametrize('metric', METRICS)
def test_graph_replay(metric):
    """Eager, capture and replays on the same buffers give identical bits, also after theta, data and labels are overwritten IN PLACE; a
    call with another scale or the other metric does not reuse the graph."""
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    _, theta2, data2, labels2, _, _, _ = _inputs('omni', (4, 5, 6, 7))
    scale = M.case_scale('omni', metric)
    other = M.COSINE if metric == M.PROTO else M.PROTO
    fresh = MetaEngine(mspec)
    call = lambda e, th, d, l, m=metric, s=scale: _np(*e.meta_batch_metric(th, d, l, shots, metric=m, scale=s, return_logits=True))
    want = call(fresh, theta, data, labels)
    want2 = call(fresh, (theta2 * 0.5).contiguous(), data2, labels2)
    want_scale = call(fresh, theta, data, labels, s=scale * 2)
    want_other = call(fresh, theta, data, labels, m=other, s=M.case_scale('omni', other))
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    th, d, l = theta.clone(), data.clone(), labels.clone()
    for i in range(3):                                     # eager, capture, replay
        _same(('replay', i), FUSED_NAMES, call(eng, th, d, l), want)
    _same('other scale', FUSED_NAMES, call(eng, th, d, l, s=scale * 2), want_scale)
    _same('other metric', FUSED_NAMES, call(eng, th, d, l, m=other, s=M.case_scale('omni', other)), want_other)
    th.copy_(theta2 * 0.5); d.copy_(data2); l.copy_(labels2)
    _same('in place', FUSED_NAMES, call(eng, th, d, l), want2)
    assert not np.array_equal(want2[0], want[0]) and not np.array_equal(want_scale[0], want[0])
    eng.set_graph(False)


@pytest.mark.parametrize('metric', METRICS)
def test_bn_export_is_the_anil_calls(metric):
    """The same trunk pass: one exported slot with the ANIL call's bits."""
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    T = data.shape[0]
    eng = MetaEngine(mspec)
    buf = eng.set_bn_export(T, 1)
    eng.meta_batch_anil(theta, data, labels, shots, 1, 0.4)
    want = _np(buf)[0]
    buf.zero_()
    eng.meta_batch_metric(theta, data, labels, shots, metric=metric, scale=M.case_scale('omni', metric))
    got = _np(buf)[0]
    assert got.shape == (1, T, 2, mspec.hidden * mspec.n_layers) and np.abs(want).sum() > 0 and np.array_equal(got, want)
    eng.set_bn_export(0)


@pytest.mark.parametrize('metric', METRICS)
def test_launch_make_up(metric):
    """Exactly one metric-head launch per call, no classifier-head or head-tangent launch, and a census that does not depend on the task
    count; the call with a gradient makes the ANIL call's launches outside the head loop (first order, one step) and nothing else."""
    seen = []
    for ids in ((0,), (0, 1, 2)):
        mspec, theta, data, labels, ways, shots, nf = _inputs('omni', ids)
        eng = MetaEngine(mspec)
        scale = M.case_scale('omni', metric)
        for with_grad in (True, False):
            c = _census(eng, lambda: eng.meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale, with_grad=with_grad))
            print(f'[census] metric call {metric}, T = {len(ids)}, with_grad {with_grad}: {sorted(c.items())}')
            assert c.get('metric_head/0') == 1 and 'head_fwd_bwd/0' not in c and 'head_tangent/0' not in c, c
            seen.append(c)
        anil = _census(eng, lambda: eng.meta_batch_anil(theta, data, labels, shots, 1, 0.4, first_order=True))
        grad = dict(seen[-2])
        assert grad.pop('metric_head/0') == 1
        for k in ('head_fwd_bwd/0', 'misc/2'):                  # the ANIL call's support pass, advance and query pass
            anil.pop(k, None)
        assert grad == anil, (grad, anil)
    assert seen[:2] == seen[2:]


def test_fused_argument_errors_come_before_any_launch():
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    eng = MetaEngine(mspec)
    T, P = data.shape[0], eng.param_count
    with pytest.raises(_lib.MiError, match='unknown metric'):
        eng.meta_batch_metric(theta, data, labels, shots, metric='euclid')
    with pytest.raises(_lib.MiError, match='scale must be positive'):
        eng.meta_batch_metric(theta, data, labels, shots, scale=0.0)
    b = C.c_size_t()
    assert eng.lib.mi_metric_workspace_bytes(eng._h, T, ways, shots, 1, C.byref(b)) == 0
    ws = eng._workspace(b.value)
    out = torch.full((P + 2 * T,), -7.0, device='cuda')
    eng.profile(True)
    args = lambda m, s: (eng._h, stream(), ptr(theta), ptr(data), ptr(labels), T, ways, shots, m, s, 1, ptr(out[P:]), ptr(out[P + T:]), ptr(out),
                         None, ptr(ws), ws.numel())
    for a, text in ((args(2, 1.0), 'unknown metric 2'), (args(-1, 1.0), 'unknown metric -1'), (args(0, 0.0), 'scale must be positive'),
                    (args(1, -2.0), 'scale must be positive'), (args(1, float('nan')), 'scale must be positive')):
        assert eng.lib.mi_meta_batch_metric(*a) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode(), eng.lib.mi_last_error(eng._h)
    pooled = MetaEngine(ModelSpec.omniglot(ways))                       # a mean-pooled head has no flattened feature vector
    with pytest.raises(_lib.MiError, match='mean-pooled'):
        pooled.meta_batch_metric(torch.zeros(pooled.param_count, device='cuda'), data, labels, shots)
    torch.cuda.synchronize()
    assert eng.profile_collect() == {} and bool((out == -7.0).all())
    eng.profile(False)


# ---------------------------------------------------------------------------------------------------------------- 6: the Python surface
@pytest.mark.parametrize('metric', METRICS)
def test_backward_fills_the_trunk_and_nothing_else(metric):
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    scale = M.case_scale('omni', metric)
    features = _trunk('omni')
    head = torch.nn.Linear(128, ways).cuda()                # a head the user also holds: untouched
    params = list(features.parameters())
    total, losses, accs = cf.meta_batch_adapt_metric(features, data, labels, shots, ways, metric=metric, scale=scale)
    assert not losses.requires_grad and tuple(losses.shape) == tuple(accs.shape) == (data.shape[0],)
    total.backward()
    l, a, g, _ = _np(*MetaEngine(mspec).meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale))
    assert np.array_equal(_grads(params), g[:nf]) and np.abs(g[:nf]).sum() > 0
    assert np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a) and total.item() == pytest.approx(float(l.sum()), rel=1e-6)
    assert head.weight.grad is None and head.bias.grad is None
    # only the sum carries the gradient
    _, losses, _ = cf.meta_batch_adapt_metric(features, data, labels, shots, ways, metric=metric, scale=scale)
    with pytest.raises(RuntimeError):
        losses.mean().backward()
    # no_grad: scores only
    with torch.no_grad():
        total, losses2, accs2 = cf.meta_batch_adapt_metric(features, data, labels, shots, ways, metric=metric, scale=scale)
    assert not total.requires_grad and np.array_equal(_np(losses2)[0], l) and np.array_equal(_np(accs2)[0], a)
    # the one-task form
    for p in params:
        p.grad = None
    loss, acc = cf.fast_adapt_metric((data[0].cpu(), labels[0].cpu()), features, shots, ways, torch.device('cuda'), metric=metric, scale=scale)
    loss.backward()
    l1, a1, g1, _ = _np(*MetaEngine(mspec).meta_batch_metric(theta, data[:1].contiguous(), labels[:1].contiguous(), shots, metric=metric, scale=scale))
    assert loss.item() == l1[0] and acc.item() == a1[0] and np.array_equal(_grads(params), g1[:nf])


def test_evaluate_nil_is_the_mean_of_the_engines_acc():
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    shape = 'omni'
    dataset, _, hw, _, ways, shots = M.SHAPES[shape]
    mspec, theta, data, labels, _, _, nf = _inputs(shape, (7, 8, 9))
    features = _trunk(shape)
    p = dict(meta_batch_size=3, shots=shots, ways=ways)
    for metric, scale in ((M.COSINE, 1.0), (M.PROTO, 0.125)):
        got = cf.evaluate_nil(p, SyntheticTasks(dataset, ways, shots, 7), features, torch.device('cuda'), metric=metric, scale=scale)
        _, acc, grad, _ = _np(*MetaEngine(mspec).meta_batch_metric(theta, data, labels, shots, metric=metric, scale=scale, with_grad=False))
        assert grad is None and got == pytest.approx(float(acc.astype(np.float64).mean()), abs=1e-6)
    # a bare ConvBase is taken as well; an OmniglotCNN is not
    assert cf.evaluate_nil(p, SyntheticTasks(dataset, ways, shots, 7), features[0], torch.device('cuda'), scale=1.0) == \
        cf.evaluate_nil(p, SyntheticTasks(dataset, ways, shots, 7), features, torch.device('cuda'), scale=1.0)
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.evaluate_nil(p, SyntheticTasks(dataset, ways, shots, 7), cf.OmniglotCNN(ways).cuda(), torch.device('cuda'))


@pytest.mark.parametrize('metric,scale', [(M.PROTO, 0.125), (M.COSINE, 4.0)])
def test_protonet_driver_trains_and_writes_anil_checkpoints(tmp_path, metric, scale):
    from exploring_meta_amd.vision import anil_vision, protonet_vision
    p = dict(protonet_vision.params)
    p.update(meta_batch_size=4, num_iterations=3, ways=5, shots=1, metric=metric, scale=scale, save_dir=str(tmp_path))
    logs = []
    features, metrics = protonet_vision.run('omni', p, log=logs.append)
    assert len(logs) == 3 and all(math.isfinite(v) for v in metrics.values()) and 'test_acc' in metrics
    torch.manual_seed(p['seed']); torch.cuda.manual_seed(p['seed'])
    init = protonet_vision.build('omni', 5, torch.device('cuda'))
    assert any(not torch.equal(a, b) for a, b in zip(features.parameters(), init.parameters()))
    assert all(torch.isfinite(q).all() for q in features.parameters())
    for name in ('features.pt', os.path.join('model_checkpoints', 'model_features_1.pt')):
        assert os.path.exists(tmp_path / name), name
    loaded, _ = anil_vision.build('omni', 5, 0.5, torch.device('cuda'))
    loaded.load_state_dict(torch.load(tmp_path / 'features.pt'))
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), features.state_dict().values()))


def test_anil_driver_nil_test_only_adds_its_key():
    from exploring_meta_amd.vision import anil_vision
    runs = []
    for nil in (False, True):
        p = dict(anil_vision.params)
        p.update(anil_vision.params_of(anil_vision.parse_args(['--meta_batch_size', '3', '--num_iterations', '2', '--shots', '1'] +
                                                               (['--nil_test'] if nil else []))))
        logs = []
        _, metrics = anil_vision.run('omni', p, log=logs.append)
        runs.append((logs, metrics))
    (l0, m0), (l1, m1) = runs
    assert 'nil_test_acc' not in m0 and len(l0) == 2
    assert l1[:len(l0)] == l0 and len(l1) == len(l0) + 1 and l1[-1].startswith('nil_test_acc: ')
    assert {k: v for k, v in m1.items() if k != 'nil_test_acc'} == m0 and 0.0 <= m1['nil_test_acc'] <= 1.0
