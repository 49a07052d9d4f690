"""The logistic-regression head on the GPU (mi_logreg_head, mi_meta_batch_logreg, include/mi_maml.h): the kernel entry
against the fp64 definition (tests/logreg_head_oracle.py: ``head``) under the bar 2^-23 + 2 e_dp + 2 e_ref, per quantity and per row, every
term from the references (e_dp = 0: the kernel keeps no intermediate in fp32; e_ref: ``closed_form`` against ``head``), at sizes on both
sides of every path the kernel takes (feat not a multiple of 4, one feature -- G of rank one --, more rows than a tile, one class, unbalanced
and absent classes, ns != nq, nq > 64, 36 ways in lanes 32 to 63 with 138880 bytes of LDS through the dynamic-LDS attribute); its exact
cases (one class, all features equal, features doubled with lam quadrupled), its bitwise relations, the NaN flag on one task of three, its
domain; the fused call against the oracle on vision_ref's trunk under every operand form; graph replay and the launch make-up; the Python
surface and the drivers."""
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
from gpu_utils import dev, ptr, rel_err, report, stream
import logreg_head_oracle as LH
import closed_form_utils as U
from closed_form_utils import census as _census, grads as _grads, held as _held, np_of as _np, same as _same

pytestmark = pytest.mark.gpu

NAMES = ('loss', 'acc', 'logits', 'dfs', 'dfq', 'dhyper')
SYMBOLS = ('mi_logreg_head_scratch_bytes', 'mi_logreg_head', 'mi_logreg_workspace_bytes', 'mi_meta_batch_logreg')

_mspec, _inputs, _trunk = (functools.partial(f, LH) for f in (U.mspec, U.inputs, U.trunk))


def _kernel(fs, fq, ys, yq, ways, lam, alpha, dfs=True, dfq=True, dhyper=True, logits=True, fill=None):
    """mi_logreg_head on numpy inputs -> (rc, numpy loss, acc, logits, dfs, dfq, dhyper); outputs the call does not take are None.  fill:
    the outputs start as this value (to see that a refused call leaves them alone)."""
    lib = _lib.load()
    fsd, fqd, ysd, yqd = dev(fs), dev(fq), dev(ys, torch.int32), dev(yq, torch.int32)
    T, ns, feat = fs.shape
    nq = fq.shape[1]
    mk = (lambda *shape: torch.full(shape, float(fill), device='cuda')) if fill is not None else (lambda *shape: torch.empty(*shape, device='cuda'))
    loss, acc = mk(T), mk(T)
    lo = mk(T, nq, ways) if logits else None
    gs = mk(T, ns, feat) if dfs else None
    gq = mk(T, nq, feat) if dfq else None
    dh = mk(T, 2) if dhyper else None
    nscr = lib.mi_logreg_head_scratch_bytes(T, ns, nq, feat, ways)
    scr = torch.empty(max(nscr, 1), dtype=torch.uint8, device='cuda')
    rc = lib.mi_logreg_head(stream(), ptr(fsd), ptr(fqd), ptr(ysd), ptr(yqd), T, ns, nq, feat, ways, float(lam), float(alpha), ptr(loss),
                            ptr(acc), ptr(lo), ptr(gs), ptr(gq), ptr(dh), ptr(scr), nscr)
    return (rc,) + _np(loss, acc, lo, gs, gq, dh)


def _check_kernel(tag, got, fs, fq, ys, yq, ways, lam, alpha):
    """Per quantity, and per row of logits, dfs and dfq: the error relative in norm against ``head`` is at most 2^-23 + 2 e_ref
    (logreg_head_oracle.bar_errors); argmax and accuracy equal on every row."""
    o64 = LH.head(fs, fq, ys, yq, ways, lam, alpha)
    *ocf, info = LH.closed_form(fs, fq, ys, yq, ways, lam, alpha)
    res = LH.bar_errors(got, o64, ocf)
    report(f'logreg_head[{tag}]', newton=info['newton'], cg=info['cg'], halvings=info['halve'],
           **{f'{n}_rel_err': float(np.max(e)) for n, (e, b) in res.items()},
           **{f'{n}_of_bar': float(np.max(e / b)) for n, (e, b) in res.items()})
    for n, (err, bar) in res.items():
        print(f'[bar] {tag} {n}: err {np.max(err):.3e}, {np.max(err / bar):.2f} of its bar')
    for n, (err, bar) in res.items():
        assert np.all(err <= bar), (tag, n, float(np.max(err)), float(np.max(err / bar)))
    assert np.array_equal(got[2].argmax(axis=-1), o64[2].argmax(axis=-1))
    assert np.array_equal(got[1], o64[1].astype(np.float32))
    return o64


# ---------------------------------------------------------------------------------------------------------------- 1: the kernel entry
@pytest.mark.parametrize('lam,alpha', LH.HYPERS)
@pytest.mark.parametrize('feat,ways,ns,nq,T', LH.ALL_CASES)
def test_kernel_against_the_fp64_definition(feat, ways, ns, nq, T, lam, alpha):
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, ns, nq, T)
    rc, *got = _kernel(fs, fq, ys, yq, ways, lam, alpha)
    assert rc == 0, _lib.load().mi_last_error(None)
    o64 = _check_kernel(f'{feat}-{ways}-{ns}/{nq}-T{T}-lam{lam:g}', got, fs, fq, ys, yq, ways, lam, alpha)
    if ways == 1:       # one class: zero Newton steps, loss exactly 0, accuracy 1, every gradient exactly 0
        assert all(np.all(g == 0) for g in (got[0], got[3], got[4], got[5])) and np.all(got[1] == 1)
    else:               # the case tests something
        assert np.all(o64[0] >= 0.05) and np.abs(o64[3]).sum() > 0 and np.abs(o64[4]).sum() > 0 and np.all(o64[5] != 0)


def _largest_rows(ways):
    n = 1
    while LH.lds_bytes(n + 1, n + 1, ways) <= 163840:
        n += 1
    return n


def test_domain_limits():
    """feat = MI_RIDGE_MAX_FEAT at ns = nq = ways = 5 computes and meets the bar; one feature more is MI_ERR_ARG naming the sizes, nothing
    launched and the outputs untouched; so is one row more than the LDS formula allows (at 20 ways)."""
    ways, n = 5, 5
    feat = LH.MAX_FEAT
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, n, n, 1)
    rc, *got = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0)
    assert rc == 0, _lib.load().mi_last_error(None)
    _check_kernel(f'limit-{feat}', got, fs, fq, ys, yq, ways, 1.0, 1.0)
    fs, fq, ys, yq = LH.kernel_inputs(feat + 1, ways, n, n, 1)
    rc, *got = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0, fill=-7.0)
    assert rc == -1
    msg = _lib.load().mi_last_error(None).decode()
    assert 'mi_logreg_head' in msg and f'feat = {feat + 1}' in msg and 'ns = 5' in msg and 'LDS' in msg, msg
    assert all(np.all(g == -7.0) for g in got)
    m = _largest_rows(20)
    assert LH.lds_bytes(m, m, 20) <= 163840 < LH.lds_bytes(m + 1, m + 1, 20) and m >= 20
    fs, fq, ys, yq = LH.kernel_inputs(8, 20, m + 1, m + 1, 1)
    rc, *got = _kernel(fs, fq, ys, yq, 20, 1.0, 1.0, fill=-7.0)
    msg = _lib.load().mi_last_error(None).decode()
    assert rc == -1 and f'ns = {m + 1}' in msg and str(LH.lds_bytes(m + 1, m + 1, 20)) in msg, msg
    assert all(np.all(g == -7.0) for g in got)


def test_argument_errors_launch_nothing():
    fs, fq, ys, yq = LH.kernel_inputs(32, 5, 5, 5, 1)
    cases = [(dict(ways=65), 'ways')]
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        cases += [(dict(lam=bad), 'lam must be positive'), (dict(alpha=bad), 'alpha must be positive')]
    for kw, text in cases:
        args = dict(ways=5, lam=1.0, alpha=1.0)
        args.update(kw)
        rc, *got = _kernel(fs, fq, ys, yq, args['ways'], args['lam'], args['alpha'], fill=-7.0)
        assert rc == -1 and text in _lib.load().mi_last_error(None).decode(), (kw, _lib.load().mi_last_error(None))
        assert all(np.all(g == -7.0) for g in got)


def test_misaligned_feature_pointers_are_refused():
    """fs, fq, dfs, dfq in turn one float into a larger buffer: MI_ERR_ARG naming the rule, nothing launched, the outputs untouched."""
    lib = _lib.load()
    feat, ways, n = 32, 5, 5
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, n, n, 1)
    ysd, yqd = dev(ys, torch.int32), dev(yq, torch.int32)
    for which in ('fs', 'fq', 'dfs', 'dfq'):
        big = {k: torch.full((n * feat + 8,), -7.0, device='cuda') for k in ('fs', 'fq', 'dfs', 'dfq')}
        v = {k: b[1:1 + n * feat] if k == which else b[4:4 + n * feat] for k, b in big.items()}
        assert all((v[k].data_ptr() % 16 == 0) == (k != which) for k in v)
        v['fs'].copy_(dev(fs).reshape(-1)); v['fq'].copy_(dev(fq).reshape(-1))
        out = torch.full((40,), -7.0, device='cuda')                          # loss at 0, acc at 4, logits (25) at 8, dhyper at 36
        rc = lib.mi_logreg_head(stream(), ptr(v['fs']), ptr(v['fq']), ptr(ysd), ptr(yqd), 1, n, n, feat, ways, 1.0, 1.0, ptr(out), ptr(out[4:]),
                                ptr(out[8:]), ptr(v['dfs']), ptr(v['dfq']), ptr(out[36:]), None, 0)
        msg = lib.mi_last_error(None).decode()
        assert rc == -1 and 'mi_logreg_head' in msg and 'must be 16-byte aligned' in msg, (which, rc, msg)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and bool((big['dfs'] == -7.0).all()) and bool((big['dfq'] == -7.0).all()), which


# ---------------------------------------------------------------------------------------------------------------- 2: exact cases
def test_all_features_equal_ties_go_to_class_zero():
    """Equal support rows with balanced classes: P is uniform, A = (Y - P) / lam, and every logit is k * sum_j A_jc = 0: all tie, the first
    maximum is class 0.  The tie is a cancellation (counts_c - ns / ways), exact in binary only where 1 / ways is: 4 classes here (at 5
    the fp64 logits are +-1e-16 of rounding noise around 0, which no rounding to fp32 collapses -- measured on the MI355X); with 4 classes,
    features of 0.25 and lam = 1 every product and sum of the solve is exact, R is exactly 0 after one Newton step and the logits are 0."""
    ways, n, feat = 4, 8, 40
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, n, n, 1)
    fs[:], fq[:] = 0.25, 0.25
    rc, loss, acc, logits, dfs, dfq, dh = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0)
    assert rc == 0 and np.isfinite(logits).all()
    assert np.all(logits == logits[..., :1]), logits                        # every logit of a row ties
    assert acc[0] == np.float32((yq[0] == 0).mean())                        # the first maximum: class 0
    assert loss[0] == pytest.approx(math.log(ways), rel=1e-6)


@pytest.mark.parametrize('feat,ways,n', [(33, 5, 5), (128, 20, 20), (1600, 5, 25)])
def test_features_doubled_lam_quadrupled(feat, ways, n):
    """(2 f, 4 lam): G is quadrupled and A quartered exactly, and every stopping rule of the solver compares scale-free quantities, so the
    two runs take the same steps -- loss, acc, logits and dalpha bit for bit, dfs and dfq exactly halved, dlam exactly quartered."""
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, n, n, 2)
    rc, *a = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0)
    rc2, *b = _kernel(2 * fs, 2 * fq, ys, yq, ways, 4.0, 1.0)
    assert rc == 0 and rc2 == 0
    _same('doubled', NAMES[:3], b[:3], a[:3])
    assert np.array_equal(b[3], a[3] / 2) and np.array_equal(b[4], a[4] / 2) and np.abs(a[3]).sum() > 0
    assert np.array_equal(b[5][:, 0], a[5][:, 0] / 4) and np.array_equal(b[5][:, 1], a[5][:, 1]) and np.all(a[5] != 0)


# ---------------------------------------------------------------------------------------------------------------- 3: bitwise relations
@pytest.mark.parametrize('feat,ways,ns,nq', [(128, 5, 5, 5), (33, 3, 6, 4), (1600, 5, 25, 25)])
def test_bitwise_relations(feat, ways, ns, nq):
    """Task t of a T = 3 call is the T = 1 call on it; forward-only is the forward half of forward + backward; seven combinations of the
    nullable outputs are accepted and change no other output."""
    fs, fq, ys, yq = LH.kernel_inputs(feat, ways, ns, nq, 3)
    rc, *whole = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0)
    assert rc == 0
    for t in range(3):
        rc, *one = _kernel(fs[t:t + 1], fq[t:t + 1], ys[t:t + 1], yq[t:t + 1], ways, 1.0, 1.0)
        assert rc == 0
        _same(('task', t), NAMES, [o[0] for o in one], [w[t] for w in whole])
    rc, *fwd = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0, dfs=False, dfq=False, dhyper=False)
    assert rc == 0 and fwd[3] is None and fwd[4] is None and fwd[5] is None
    _same('forward only', NAMES[:3], fwd[:3], whole[:3])
    for kw in (dict(logits=False), dict(dhyper=False), dict(dfs=False), dict(dfq=False), dict(dfs=False, dfq=False),
               dict(dfs=False, dfq=False, dhyper=False, logits=False), dict(dfq=False, dhyper=False, logits=False)):
        rc, *part = _kernel(fs, fq, ys, yq, ways, 1.0, 1.0, **kw)
        assert rc == 0
        for name, a, b in zip(NAMES, part, whole):
            assert (a is None) == (not kw.get(name, True)) and (a is None or np.array_equal(a, b)), (kw, name)


def test_task_independence_beyond_the_cu_count():
    """257 tasks, one more than the 256 CUs: every task of the one launch is the T = 1 call on it, bit for bit."""
    T = 257
    fs, fq, ys, yq = LH.kernel_inputs(8, 5, 5, 5, T)
    rc, *whole = _kernel(fs, fq, ys, yq, 5, 1.0, 1.0)
    assert rc == 0 and all(np.isfinite(w).all() for w in whole) and len({w.tobytes() for w in whole[3]}) == T
    for t in range(T):
        rc, *one = _kernel(fs[t:t + 1], fq[t:t + 1], ys[t:t + 1], yq[t:t + 1], 5, 1.0, 1.0)
        assert rc == 0
        _same(('task', t), NAMES, [o[0] for o in one], [w[t] for w in whole])


def test_a_residual_that_is_not_finite_flags_its_task_alone():
    """The header's flag (no fault: no loop bound and no address of the kernel depends on data).  A NaN in one element of task 1's fs makes
    its residual NaN at the first trial step: every output of that task is NaN, in the forward-only launch too; tasks 0 and 2 are finite
    and the bits of their T = 1 calls."""
    fs, fq, ys, yq = LH.flag_inputs()
    rc, *whole = _kernel(fs, fq, ys, yq, 2, 1.0, 1.0, fill=-7.0)
    assert rc == 0, _lib.load().mi_last_error(None)
    for name, w in zip(NAMES, whole):
        assert np.all(np.isnan(w[1])), (name, w[1])
    for t in (0, 2):
        rc, *one = _kernel(fs[t:t + 1], fq[t:t + 1], ys[t:t + 1], yq[t:t + 1], 2, 1.0, 1.0)
        assert rc == 0 and all(np.isfinite(w[t]).all() for w in whole)
        _same(('task', t), NAMES, [o[0] for o in one], [w[t] for w in whole])
    rc, *fwd = _kernel(fs, fq, ys, yq, 2, 1.0, 1.0, dfs=False, dfq=False, dhyper=False, fill=-7.0)
    assert rc == 0 and all(np.all(np.isnan(w[1])) for w in fwd[:3])
    _same('forward only', NAMES[:3], [w[::2] for w in fwd[:3]], [w[::2] for w in whole[:3]])


# ---------------------------------------------------------------------------------------------------------------- 4: the fused call
@functools.lru_cache(maxsize=None)
def _oracle(shape, fp64, ids=None):
    """One oracle run per case and precision, shared by every test that needs it (never modified)."""
    return LH.case_oracle(shape, ids, torch.float64 if fp64 else torch.float32)


def _check_fused(tag, shape, got, nf, ids=None):
    loss, acc, grad, dh, logits = got
    o64, o32 = _oracle(shape, True, ids), _oracle(shape, False, ids)
    l64, h64 = o64['losses'], o64['dhyper'].sum(axis=0)
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), trunk=rel_err(grad[:nf], o64['grad_feat']),
                dhyper=np.abs(dh.astype(np.float64).sum(axis=0) - h64) / np.abs(h64))
    refs = dict(loss=np.abs(o32['losses'] - l64) / np.abs(l64), trunk=rel_err(o32['grad_feat'], o64['grad_feat']),
                dhyper=np.abs(o32['dhyper'].sum(axis=0) - h64) / np.abs(h64))
    report(f'logreg_fused[{shape}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           trunk_rel_err=errs['trunk'], ref_fp32_trunk_rel_err=refs['trunk'], dlam_rel_err=float(errs['dhyper'][0]),
           ref_fp32_dlam_rel_err=float(refs['dhyper'][0]), dalpha_rel_err=float(errs['dhyper'][1]), ref_fp32_dalpha_rel_err=float(refs['dhyper'][1]))
    _held('loss', errs['loss'], refs['loss'], LH.LOSS_FLOOR)
    _held('trunk', errs['trunk'], refs['trunk'], LH.GRAD_FLOOR[shape])
    _held('dhyper', errs['dhyper'], refs['dhyper'], LH.HYPER_FLOOR)
    assert grad.shape[0] > nf and np.all(grad[nf:] == 0)                     # the head's entries: exact zeros
    clear = LH.clear_rows(o64['logits'][None])[0]
    assert clear.all()                                                       # (tests/test_logreg_head_host.py chose lam and alpha so)
    assert np.array_equal(logits.argmax(axis=-1), o64['logits'].argmax(axis=-1))
    assert np.array_equal(acc, o64['accs'].astype(np.float32))


@pytest.mark.parametrize('shape', list(LH.FUSED_CASES))
def test_fused_call_against_the_fp64_oracle(conv_form, shape):
    """Every operand form: loss and the summed dhyper within max(1e-4, 2 x the fp32 oracle's error), the trunk gradient within max(the
    ANIL bar of the same trunk, 2 x the fp32 oracle's error), argmax and accuracy equal, the head's gradient entries exactly zero (theta's
    head entries are NaN: they are not read).  with_grad = 0: loss, acc and logits bit for bit, meta_grad_out and dhyper_out untouched."""
    mspec, theta, data, labels, ways, shots, nf = _inputs(shape, head=float('nan'))
    eng = MetaEngine(mspec)
    _, lam, alpha = LH.FUSED_CASES[shape]
    got = _np(*eng.meta_batch_logreg(theta, data, labels, shots, lam=lam, scale=alpha, return_logits=True))
    _check_fused(conv_form, shape, got, nf)
    # evaluation only, through the C entry so that meta_grad_out and dhyper_out are buffers of ours
    T, n = data.shape[0], ways * shots
    b = C.c_size_t()
    assert eng.lib.mi_logreg_workspace_bytes(eng._h, T, ways, shots, 0, C.byref(b)) == 0
    ws = eng._workspace(b.value)
    P = eng.param_count
    out = torch.full((P + 2 * T + 2 * T + T * n * ways,), -7.0, device='cuda')
    rc = eng.lib.mi_meta_batch_logreg(eng._h, stream(), ptr(theta), ptr(data), ptr(labels), T, ways, shots, lam, alpha, 0, ptr(out[P:]),
                                      ptr(out[P + T:]), ptr(out), ptr(out[P + 2 * T:]), ptr(out[P + 4 * T:]), ptr(ws), ws.numel())
    assert rc == 0, eng.lib.mi_last_error(eng._h)
    o = _np(out)[0]
    assert np.all(o[:P] == -7.0) and np.all(o[P + 2 * T:P + 4 * T] == -7.0)
    _same('with_grad=0', ('loss', 'acc', 'logits'), (o[P:P + T], o[P + T:P + 2 * T], o[P + 4 * T:].reshape(T, n, ways)), (got[0], got[1], got[4]))


def test_fused_call_single_task():
    """omni at T = 1 (task 0): the oracle's bars, and the bits of task 0 of the four-task call's loss, acc, dhyper and logits."""
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni', (0,))
    eng = MetaEngine(mspec)
    _, lam, alpha = LH.FUSED_CASES['omni']
    got = _np(*eng.meta_batch_logreg(theta, data, labels, shots, lam=lam, scale=alpha, return_logits=True))
    _check_fused('T1', 'omni', got, nf, ids=(0,))
    _, _, data4, labels4, _, _, _ = _inputs('omni')
    whole = _np(*eng.meta_batch_logreg(theta, data4, labels4, shots, lam=lam, scale=alpha, return_logits=True))
    _same('task 0', ('loss', 'acc', 'dhyper', 'logits'), [got[i][0] for i in (0, 1, 3, 4)], [whole[i][0] for i in (0, 1, 3, 4)])


# ---------------------------------------------------------------------------------------------------------------- 5: engine behaviour
FUSED_NAMES = ('loss', 'acc', 'grad', 'dhyper', 'logits')


def test_graph_replay():
    """Eager, capture and replays on the same buffers give identical bits, also after theta, data and labels are overwritten IN PLACE; a
    call with another lam or another alpha does not reuse the graph."""
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    _, theta2, data2, labels2, _, _, _ = _inputs('omni', (4, 5, 6, 7))
    _, lam, alpha = LH.FUSED_CASES['omni']
    fresh = MetaEngine(mspec)
    call = lambda e, th, d, l, lm=lam, al=alpha: _np(*e.meta_batch_logreg(th, d, l, shots, lam=lm, scale=al, return_logits=True))
    want = call(fresh, theta, data, labels)
    want2 = call(fresh, (theta2 * 0.5).contiguous(), data2, labels2)
    want_lam = call(fresh, theta, data, labels, lm=lam * 2)
    want_alpha = call(fresh, theta, data, labels, al=alpha * 2)
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    th, d, l = theta.clone(), data.clone(), labels.clone()
    for i in range(3):                                     # eager, capture, replay
        _same(('replay', i), FUSED_NAMES, call(eng, th, d, l), want)
    _same('other lam', FUSED_NAMES, call(eng, th, d, l, lm=lam * 2), want_lam)
    _same('other alpha', FUSED_NAMES, call(eng, th, d, l, al=alpha * 2), want_alpha)
    _same('back', FUSED_NAMES, call(eng, th, d, l), want)
    th.copy_(theta2 * 0.5); d.copy_(data2); l.copy_(labels2)
    _same('in place', FUSED_NAMES, call(eng, th, d, l), want2)
    assert not np.array_equal(want2[0], want[0]) and not np.array_equal(want_lam[0], want[0]) and not np.array_equal(want_alpha[0], want[0])
    assert all(np.isfinite(w).all() for w in want + want2)
    eng.set_graph(False)


def test_launch_make_up():
    """Exactly one logreg_head/0 launch per call, whatever the task count; apart from it the launches are mi_meta_batch_metric's."""
    seen = []
    for ids in ((0,), (0, 1, 2)):
        mspec, theta, data, labels, ways, shots, nf = _inputs('omni', ids)
        eng = MetaEngine(mspec)
        for with_grad in (True, False):
            c = _census(eng, lambda: eng.meta_batch_logreg(theta, data, labels, shots, lam=1.0, scale=1.0, with_grad=with_grad))
            m = _census(eng, lambda: eng.meta_batch_metric(theta, data, labels, shots, metric='proto', scale=0.125, with_grad=with_grad))
            print(f'[census] logreg call, T = {len(ids)}, with_grad {with_grad}: {sorted(c.items())}')
            assert c.get('logreg_head/0') == 1 and not {'metric_head/0', 'ridge_head/0', 'head_fwd_bwd/0'} & set(c), c
            seen.append(dict(c))
            assert c.pop('logreg_head/0') == 1 and m.pop('metric_head/0') == 1 and c == m, (c, m)
    assert seen[:2] == seen[2:]


def test_fused_argument_errors_come_before_any_launch():
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    eng = MetaEngine(mspec)
    T, P = data.shape[0], eng.param_count
    with pytest.raises(_lib.MiError, match='lam must be positive'):
        eng.meta_batch_logreg(theta, data, labels, shots, lam=0.0)
    with pytest.raises(_lib.MiError, match='scale must be positive'):
        eng.meta_batch_logreg(theta, data, labels, shots, scale=-1.0)
    b = C.c_size_t()
    assert eng.lib.mi_logreg_workspace_bytes(eng._h, T, ways, shots, 1, C.byref(b)) == 0
    ws = eng._workspace(b.value)
    out = torch.full((P + 4 * T,), -7.0, device='cuda')
    eng.profile(True)
    args = lambda lm, al: (eng._h, stream(), ptr(theta), ptr(data), ptr(labels), T, ways, shots, lm, al, 1, ptr(out[P:]), ptr(out[P + T:]),
                           ptr(out), ptr(out[P + 2 * T:]), None, ptr(ws), ws.numel())
    for a, text in ((args(0.0, 1.0), 'lam must be positive'), (args(float('nan'), 1.0), 'lam must be positive'),
                    (args(1.0, -1.0), 'alpha must be positive'), (args(1.0, float('inf')), 'alpha must be positive')):
        assert eng.lib.mi_meta_batch_logreg(*a) == -1
        msg = eng.lib.mi_last_error(eng._h).decode()
        assert text in msg and 'mi_meta_batch_logreg' in msg, msg
    pooled = MetaEngine(ModelSpec.omniglot(ways))                       # a mean-pooled head has no flattened feature vector
    with pytest.raises(_lib.MiError, match='mean-pooled'):
        pooled.meta_batch_logreg(torch.zeros(pooled.param_count, device='cuda'), data, labels, shots)
    torch.cuda.synchronize()
    assert eng.profile_collect() == {} and bool((out == -7.0).all())
    eng.profile(False)


# ---------------------------------------------------------------------------------------------------------------- 6: the Python surface
def test_backward_fills_the_trunk_and_the_heads_two_scalars():
    mspec, theta, data, labels, ways, shots, nf = _inputs('omni')
    features = _trunk('omni')
    head = cf.LogRegHead(lam=2.0, scale=1.5).cuda()
    lam, alpha = head.lam, head.scale
    params = list(features.parameters())
    total, losses, accs = cf.meta_batch_adapt_logreg(features, head, data, labels, shots, ways)
    assert not losses.requires_grad and tuple(losses.shape) == tuple(accs.shape) == (data.shape[0],)
    total.backward()
    l, a, g, dh, _ = _np(*MetaEngine(mspec).meta_batch_logreg(theta, data, labels, shots, lam=lam, scale=alpha))
    assert np.array_equal(_grads(params), g[:nf]) and np.abs(g[:nf]).sum() > 0
    assert np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a) and total.item() == pytest.approx(float(l.sum()), rel=1e-6)
    # the chain rule d/dlog x = x d/dx on the sum of the per-task rows
    hs = dh.astype(np.float64).sum(axis=0)
    assert hs[0] != 0 and hs[1] != 0                       # (rel 1e-6: one fp32 rounding of the product, whatever the order of the fp64 sum)
    assert head.log_lam.grad.item() == pytest.approx(hs[0] * lam, rel=1e-6) and head.log_scale.grad.item() == pytest.approx(hs[1] * alpha, rel=1e-6)
    # only the sum carries the gradient
    _, losses, _ = cf.meta_batch_adapt_logreg(features, head, data, labels, shots, ways)
    with pytest.raises(RuntimeError):
        losses.mean().backward()
    # no_grad: scores only
    with torch.no_grad():
        total, losses2, accs2 = cf.meta_batch_adapt_logreg(features, head, data, labels, shots, ways)
    assert not total.requires_grad and np.array_equal(_np(losses2)[0], l) and np.array_equal(_np(accs2)[0], a)
    # a fixed head: the trunk alone gets a gradient
    for p in params:
        p.grad = None
    fixed = cf.LogRegHead(lam=2.0, scale=1.5, learnable=False).cuda()
    cf.meta_batch_adapt_logreg(features, fixed, data, labels, shots, ways)[0].backward()
    assert np.array_equal(_grads(params), g[:nf])
    # the one-task form
    for p in params + list(head.parameters()):
        p.grad = None
    loss, acc = cf.fast_adapt_logreg((data[0].cpu(), labels[0].cpu()), features, head, shots, ways, torch.device('cuda'))
    loss.backward()
    l1, a1, g1, dh1, _ = _np(*MetaEngine(mspec).meta_batch_logreg(theta, data[:1].contiguous(), labels[:1].contiguous(), shots, lam=lam, scale=alpha))
    assert loss.item() == l1[0] and acc.item() == a1[0] and np.array_equal(_grads(params), g1[:nf])
    assert head.log_lam.grad.item() == pytest.approx(float(dh1[0, 0]) * lam, rel=1e-6)
    assert head.log_scale.grad.item() == pytest.approx(float(dh1[0, 1]) * alpha, rel=1e-6)
    # the ridge entries do not take this head's place silently, nor the other way round
    with pytest.raises(TypeError, match='LogRegHead'):
        cf.meta_batch_adapt_logreg(features, cf.RidgeHead(), data, labels, shots, ways)


def test_evaluate_logreg_is_the_mean_of_the_engines_acc(capsys):
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    shape = 'omni'
    dataset, _, hw, _, ways, shots = LH.SHAPES[shape]
    mspec, theta, data, labels, _, _, nf = _inputs(shape, (7, 8, 9))
    features = _trunk(shape)
    p = dict(meta_batch_size=3, shots=shots, ways=ways)
    head = cf.LogRegHead(lam=1.0, scale=1.0, learnable=False)
    got = cf.evaluate_logreg(p, SyntheticTasks(dataset, ways, shots, 7), features, head, torch.device('cuda'))
    assert 'LogReg Test Accuracy' in capsys.readouterr().out
    _, acc, grad, dh, _ = _np(*MetaEngine(mspec).meta_batch_logreg(theta, data, labels, shots, lam=head.lam, scale=head.scale, with_grad=False))
    assert grad is None and dh is None and got == pytest.approx(float(acc.astype(np.float64).mean()), abs=1e-6)
    with pytest.raises(NotImplementedError, match='OmniglotCNN'):
        cf.evaluate_logreg(p, SyntheticTasks(dataset, ways, shots, 7), cf.OmniglotCNN(ways).cuda(), head, torch.device('cuda'))


def test_logreg_driver_runs_saves_and_reloads(tmp_path):
    """Two optimisation steps on synthetic Omniglot tasks: nothing in particular gets lower, but the run moves the trunk and the head's
    two scalars, saves them under the ANIL driver's names and reloads."""
    from exploring_meta_amd.vision import anil_vision, logreg_vision
    p = dict(logreg_vision.params)
    p.update(meta_batch_size=4, num_iterations=2, ways=5, shots=1, lam=1.0, scale=2.0, save_dir=str(tmp_path))
    logs = []
    (features, head), metrics = logreg_vision.run('omni', p, log=logs.append)
    assert len(logs) == 2 and all(math.isfinite(v) for v in metrics.values()) and 'test_acc' in metrics
    torch.manual_seed(p['seed']); torch.cuda.manual_seed(p['seed'])
    init, _ = logreg_vision.build('omni', 5, torch.device('cuda'))
    assert any(not torch.equal(a, b) for a, b in zip(features.parameters(), init.parameters()))
    assert all(torch.isfinite(q).all() for q in features.parameters())
    assert head.lam != 1.0 and head.scale != 2.0 and math.isfinite(head.lam) and math.isfinite(head.scale)
    for name in ('features.pt', 'logreg_head.pt', os.path.join('model_checkpoints', 'model_features_1.pt'),
                 os.path.join('model_checkpoints', 'model_logreg_head_1.pt')):
        assert os.path.exists(tmp_path / name), name
    loaded, _ = anil_vision.build('omni', 5, 0.5, torch.device('cuda'))
    loaded.load_state_dict(torch.load(tmp_path / 'features.pt'))
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), features.state_dict().values()))
    again = cf.LogRegHead()
    again.load_state_dict(torch.load(tmp_path / 'logreg_head.pt'))
    assert again.lam == head.lam and again.scale == head.scale
    # --fix_head: the two scalars stay where they were put
    p.update(fix_head=True, save_dir='')
    (_, fixed), _ = logreg_vision.run('omni', p, log=logs.append)
    assert fixed.lam == pytest.approx(1.0, rel=1e-6) and fixed.scale == pytest.approx(2.0, rel=1e-6) and list(fixed.parameters()) == []


def test_anil_driver_logreg_test_only_adds_its_key():
    from exploring_meta_amd.vision import anil_vision
    runs = []
    for logreg in (False, True):
        p = dict(anil_vision.params)
        p.update(anil_vision.params_of(anil_vision.parse_args(['--meta_batch_size', '3', '--num_iterations', '2', '--shots', '1'] +
                                                               (['--logreg_test', '--logreg_lam', '2'] if logreg else []))))
        logs = []
        _, metrics = anil_vision.run('omni', p, log=logs.append)
        runs.append((logs, metrics))
    (l0, m0), (l1, m1) = runs
    assert 'logreg_test_acc' not in m0 and len(l0) == 2
    assert l1[:len(l0)] == l0 and len(l1) == len(l0) + 1 and l1[-1].startswith('logreg_test_acc: ')
    assert {k: v for k, v in m1.items() if k != 'logreg_test_acc'} == m0 and 0.0 <= m1['logreg_test_acc'] <= 1.0


def test_the_library_exports_every_symbol_the_header_declares():
    U.symbols_declared_and_bound(SYMBOLS)
    lib = _lib.load()
    assert all(callable(getattr(lib, s)) for s in SYMBOLS)
