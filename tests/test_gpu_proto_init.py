"""The Proto-MAML head initialisation on the GPU (mi_proto_init, mi_proto_init_bwd, mi_meta_batch_anil_proto, include/mi_maml.h; DESIGN.md
section 30): the two kernel entries against the fp64 oracle of the definitions (tests/proto_init_oracle.py) at sizes on both sides of every
path they take (feat not a multiple of 4, more than one sweep of the columns, one class, unbalanced classes, 64 classes), their exact
properties and domain; the fused call against the autograd oracle whose theta_0 is built inside the graph, at K = 0 also against the
merged metric head; graph replay, the launch make-up; the Python surface and the driver.
The edge cases (proto_init_oracle.EDGE_CASES) run what the cases above do not: the 16-byte forward loop past column 1024 and the vector
backward with more items than threads (stride 4116), a partial last chunk after the wrap, classes without a support row (W_0 = 0, b_0 = 0,
no gradient); the same bits from bases one float off a 16-byte boundary; 257 tasks against their T = 1 calls."""
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
import proto_init_oracle as P
import closed_form_utils as U
from closed_form_utils import census as _census, grads as _grads, held as _held, np_of as _np, same as _same

pytestmark = pytest.mark.gpu

KERNEL_FLOOR = 4 * 2.0 ** -24      # the handful of roundings a store and a short sum must make
NAN = float('nan')

_mspec, _inputs, _trunk = (functools.partial(f, P) for f in (U.mspec, U.inputs, U.trunk))


def _w(*ws):
    return torch.tensor(ws, dtype=torch.float32, device='cuda')


def _err():
    return _lib.load().mi_last_error(None).decode()


def _shifted(t, off):
    """t's values in a buffer of its own that starts `off` floats past an allocation's (16-byte aligned) base."""
    if not off:
        return t
    big = torch.empty(t.numel() + off, dtype=t.dtype, device='cuda')
    view = big[off:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


def _fwd(fs, ys, ways, scale, fill=None, pad=0, off=0):
    """mi_proto_init on numpy inputs -> (rc, head [T, Ph] numpy); pad: extra floats between the tasks' heads; off: fs and head_out start
    this many floats past a 16-byte boundary."""
    T, ns, feat = fs.shape
    ph = ways * feat + ways
    fsd, ysd = _shifted(dev(fs), off), dev(ys, torch.int32)
    head = _shifted(torch.full((T, ph + pad), float(fill if fill is not None else 0.0), device='cuda'), off)
    rc = _lib.load().mi_proto_init(stream(), ptr(fsd), ptr(ysd), T, ns, feat, ways, float(scale), ptr(head), ph + pad)
    return rc, _np(head)[0][:, :ph]


def _bwd(fs, ys, lam, ways, scale, dfs0, want_dscale=True, fill=None, off=0):
    """mi_proto_init_bwd -> (rc, dfs, dscale or None); off: fs, lam_head and dfs start this many floats past a 16-byte boundary."""
    T, ns, feat = fs.shape
    fsd, ysd, lamd, dfs = _shifted(dev(fs), off), dev(ys, torch.int32), _shifted(dev(lam), off), _shifted(dev(dfs0).clone(), off)
    dscale = torch.full((T,), float(fill if fill is not None else 0.0), device='cuda') if want_dscale else None
    rc = _lib.load().mi_proto_init_bwd(stream(), ptr(fsd), ptr(ysd), ptr(lamd), lam.shape[1], T, ns, feat, ways, float(scale), ptr(dfs), ptr(dscale))
    return (rc,) + _np(dfs, dscale)


# ---------------------------------------------------------------------------------------------------------------- 1: the kernel entries
@pytest.mark.parametrize('feat,ways,ns,T', P.KERNEL_CASES + P.EDGE_CASES)
def test_kernels_against_the_fp64_oracle(feat, ways, ns, T):
    """W_0, b_0, dfs and dscale each within max(2 x the fp32 autograd oracle's own error against fp64, 4 * 2^-24), relative in norm."""
    fs, ys, lam, dfs0 = P.kernel_inputs(feat, ways, ns, T)
    scale = 1.0 / feat
    rc, head = _fwd(fs, ys, ways, scale)
    assert rc == 0, _err()
    rc, dfs, dscale = _bwd(fs, ys, lam, ways, scale, dfs0)
    assert rc == 0, _err()
    o64, o32 = (P.init_autograd(fs, ys, lam, ways, scale, dt) for dt in (torch.float64, torch.float32))
    nw = ways * feat
    split = lambda o: dict(W0=o[0][:, :nw], b0=o[0][:, nw:], dfs=dfs0.astype(o[1].dtype) + o[1], dscale=o[2])
    want, ref = split(o64), split(o32)
    got = dict(W0=head[:, :nw], b0=head[:, nw:], dfs=dfs, dscale=dscale)
    errs = {n: rel_err(got[n], want[n]) for n in got}
    refs = {n: rel_err(ref[n], want[n]) for n in got}
    report(f'proto_init[{feat}-{ways}-{ns}-T{T}]', **{f'{n}_rel_err': e for n, e in errs.items()}, **{f'ref_fp32_{n}_rel_err': e for n, e in refs.items()})
    for n in errs:
        _held(f'{feat}-{ways}-{ns}-T{T} {n}', errs[n], refs[n], KERNEL_FLOOR)
    assert np.abs(want['W0']).sum() > 0 and np.abs(o64[1]).sum() > 0 and np.all(np.abs(want['dscale']) > 0)      # the case tests something


def test_exact_properties_of_the_kernels():
    """fs * 2 with scale / 4: W_0 exactly halved, b_0 bit for bit.  Task t of a T = 3 call is the T = 1 call bit for bit, whatever the
    stride between the heads.  dscale = NULL changes no other output."""
    feat, ways, ns, T = 132, 5, 10, 3
    fs, ys, lam, dfs0 = P.kernel_inputs(feat, ways, ns, T)
    scale = 1.0 / 33
    rc, head = _fwd(fs, ys, ways, scale)
    rc2, head2 = _fwd(2 * fs, ys, ways, np.float32(scale) / 4)
    assert rc == 0 and rc2 == 0, _err()
    nw = ways * feat
    assert np.array_equal(head2[:, :nw], head[:, :nw] / 2) and np.array_equal(head2[:, nw:], head[:, nw:]) and np.abs(head).min() > 0
    _, dfs, dscale = _bwd(fs, ys, lam, ways, scale, dfs0)
    rc, dfs_n, none = _bwd(fs, ys, lam, ways, scale, dfs0, want_dscale=False)
    assert rc == 0 and none is None and np.array_equal(dfs_n, dfs) and not np.array_equal(dfs, dfs0)
    for t in range(T):
        one = slice(t, t + 1)
        _, h1 = _fwd(fs[one], ys[one], ways, scale, pad=3)           # (an odd stride: the word path, the same bits)
        _, d1, s1 = _bwd(fs[one], ys[one], lam[one], ways, scale, dfs0[one])
        assert np.array_equal(h1[0], head[t]) and np.array_equal(d1[0], dfs[t]) and np.array_equal(s1[0], dscale[t])
    # the labels select the rows: another labelling of the same features gives another head
    assert not np.array_equal(_fwd(fs, ys[:, ::-1].copy(), ways, scale)[1], head)


def test_a_class_without_a_support_row():
    """What the header states for N_w = 0 (outside the definition, never a fault): with ys = (0, 2, 4) of 5 classes, rows 1 and 3 of W_0 and
    entries 1 and 3 of b_0 are exactly 0 (the other rows are not), and dfs and dscale are the oracle's, which gives such a class no gradient
    (test_kernels_against_the_fp64_oracle holds the same case to the bars)."""
    feat, ways, ns = 515, 5, 3
    fs, ys, lam, dfs0 = P.kernel_inputs(feat, ways, ns, 1)
    assert ys[0].tolist() == [0, 2, 4]
    rc, head = _fwd(fs, ys, ways, 1.0 / feat, fill=-7.0)
    assert rc == 0, _err()
    w0, b0 = head[0, :ways * feat].reshape(ways, feat), head[0, ways * feat:]
    assert np.all(w0[[1, 3]] == 0) and np.all(b0[[1, 3]] == 0) and np.all(w0[[0, 2, 4]] != 0) and np.all(b0[[0, 2, 4]] < 0)
    # the cotangent of an absent class enters nothing: another lamW[1], lamb[3] gives the same bits
    rc, dfs, dscale = _bwd(fs, ys, lam, ways, 1.0 / feat, dfs0)
    lam2 = lam.copy()
    lam2[0, feat:2 * feat] += 1.0
    lam2[0, ways * feat + 3] -= 2.0
    rc2, dfs2, dscale2 = _bwd(fs, ys, lam2, ways, 1.0 / feat, dfs0)
    assert rc == 0 and rc2 == 0 and np.array_equal(dfs2, dfs) and np.array_equal(dscale2, dscale) and not np.array_equal(dfs, dfs0)


def test_bits_do_not_depend_on_the_alignment_of_the_bases():
    """(132, 4, 8) at T = 2, stride 532: every row on a 16-byte boundary takes the 16-byte path; fs, head_out, lam_head and dfs each one float
    into a larger buffer take the word path -- W_0, b_0, dfs and dscale bit for bit."""
    feat, ways, ns, T = 132, 4, 8, 2
    fs, ys, lam, dfs0 = P.kernel_inputs(feat, ways, ns, T)
    assert (ways * feat + ways) % 4 == 0 and feat % 4 == 0
    scale = 1.0 / feat
    rc, head = _fwd(fs, ys, ways, scale)
    rc1, head1 = _fwd(fs, ys, ways, scale, off=1)
    assert rc == 0 and rc1 == 0, _err()
    assert np.array_equal(head1, head) and np.abs(head).min() > 0
    rc, dfs, dscale = _bwd(fs, ys, lam, ways, scale, dfs0)
    rc1, dfs1, dscale1 = _bwd(fs, ys, lam, ways, scale, dfs0, off=1)
    assert rc == 0 and rc1 == 0, _err()
    assert np.array_equal(dfs1, dfs) and np.array_equal(dscale1, dscale) and not np.array_equal(dfs, dfs0) and np.all(dscale != 0)


def test_task_independence_beyond_the_cu_count():
    """257 tasks, one more than the 256 CUs (1285 forward workgroups): every task of the one launch is the T = 1 call on it, bit for bit."""
    feat, ways, ns, T = 8, 5, 5, 257
    fs, ys, lam, dfs0 = P.kernel_inputs(feat, ways, ns, T)
    scale = 1.0 / feat
    rc, head = _fwd(fs, ys, ways, scale)
    rc2, dfs, dscale = _bwd(fs, ys, lam, ways, scale, dfs0)
    assert rc == 0 and rc2 == 0, _err()
    assert len({h.tobytes() for h in head}) == T and np.isfinite(head).all() and np.isfinite(dfs).all()
    for t in range(T):
        one = slice(t, t + 1)
        rc, h1 = _fwd(fs[one], ys[one], ways, scale)
        rc2, d1, s1 = _bwd(fs[one], ys[one], lam[one], ways, scale, dfs0[one])
        assert rc == 0 and rc2 == 0
        assert np.array_equal(h1[0], head[t]) and np.array_equal(d1[0], dfs[t]) and np.array_equal(s1[0], dscale[t]), t


def test_domain_errors_launch_nothing():
    """scale 0, -1, NaN, inf; ways = 65; feat = MI_RIDGE_MAX_FEAT + 1: MI_ERR_ARG naming the sizes, the outputs untouched."""
    fs, ys, lam, dfs0 = P.kernel_inputs(32, 5, 5, 1)
    for scale in (0.0, -1.0, NAN, float('inf')):
        rc, head = _fwd(fs, ys, 5, scale, fill=-7.0)
        assert rc == -1 and 'mi_proto_init: scale must be positive and finite' in _err() and np.all(head == -7.0)
        rc, dfs, dscale = _bwd(fs, ys, lam, 5, scale, dfs0, fill=-7.0)
        assert rc == -1 and 'mi_proto_init_bwd: scale must be positive and finite' in _err() and np.array_equal(dfs, dfs0) and np.all(dscale == -7.0)
    big = np.zeros((1, 65 * 32 + 65), np.float32)
    rc, head = _fwd(fs, ys, 65, 1.0, fill=-7.0)
    assert rc == -1 and 'ways = 65' in _err() and 'ways in 1..64' in _err() and np.all(head == -7.0)
    rc, dfs, dscale = _bwd(fs, ys, big, 65, 1.0, dfs0, fill=-7.0)
    assert rc == -1 and 'ways = 65' in _err() and np.array_equal(dfs, dfs0) and np.all(dscale == -7.0)
    feat = P.MAX_FEAT + 1
    wide, y1 = np.ones((1, 1, feat), np.float32), np.zeros((1, 1), np.int32)
    rc, head = _fwd(wide, y1, 1, 1.0, fill=-7.0)
    assert rc == -1 and f'feat = {feat}' in _err() and f'feat in 1..{P.MAX_FEAT}' in _err() and np.all(head == -7.0)
    rc, dfs, dscale = _bwd(wide, y1, np.ones((1, feat + 1), np.float32), 1, 1.0, np.zeros_like(wide), fill=-7.0)
    assert rc == -1 and f'feat = {feat}' in _err() and np.all(dfs == 0) and np.all(dscale == -7.0)
    rc, head = _fwd(wide[:, :, :-1], y1, 1, 1.0)                    # the cap itself computes: W_0 = 2 c, b_0 = -|c|^2
    assert rc == 0 and np.all(head[0, :-1] == 2.0) and head[0, -1] == -float(P.MAX_FEAT)


# ---------------------------------------------------------------------------------------------------------------- 2: the fused call
@functools.lru_cache(maxsize=None)
def _oracle(case, fp64):
    """One oracle run per case and precision, shared by every test that needs it (never modified)."""
    return P.case_oracle(case, torch.float64 if fp64 else torch.float32)


def _step_args(case):
    lr = P.case_lr(case)
    return dict(inner_lr=float(lr)) if np.ndim(lr) == 0 else dict(lr_vec=dev(lr))


def _run_case(eng, case, **kw):
    """(loss, acc, grad, lr_grad, dscale, logits) numpy; the learner's head in theta is NaN: it enters no result."""
    shape, _, K, kind, fo, w = P.FUSED[case]
    _, theta, data, labels, _, shots, _ = _inputs(shape, P.case_ids(case), head=NAN)
    return _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, P.CASES[shape][1], step_w=None if w is None else _w(*w), first_order=fo,
                                          want_lr_grad=kind != 'scalar', return_logits=True, **_step_args(case), **kw))


def _check_vs_oracle(tag, case, got):
    loss, acc, grad, lr_grad, dscale, logits = got
    shape, _, K, kind, _, w = P.FUSED[case]
    o64, o32 = _oracle(case, True), _oracle(case, False)
    rows = slice(K, K + 1) if w is None else slice(0, K + 1)
    if w is None:
        loss, acc, logits = loss[None], acc[None], logits[None]
    l64 = o64['losses'][rows]
    nf = o64['grad_feat'].size
    rel = lambda a, b: abs(a - b) / abs(b)
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), trunk=rel_err(grad[:nf], o64['grad_feat']), dscale=rel(float(dscale.astype(np.float64).sum()), o64['dscale']))
    refs = dict(loss=np.abs(o32['losses'][rows] - l64) / np.abs(l64), trunk=rel_err(o32['grad_feat'], o64['grad_feat']), dscale=rel(o32['dscale'], o64['dscale']))
    if kind != 'scalar':
        assert lr_grad.shape == o64['lr_grad'].shape
        errs['lr_grad'], refs['lr_grad'] = rel_err(lr_grad, o64['lr_grad']), rel_err(o32['lr_grad'], o64['lr_grad'])
    report(f'proto_anil[{case}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           **{f'{n}_rel_err': errs[n] for n in errs if n != 'loss'}, **{f'ref_fp32_{n}_rel_err': refs[n] for n in refs if n != 'loss'},
           dscale_tasks_rel_err=rel_err(dscale, o64['dscale_tasks']))
    _held('loss', errs['loss'], refs['loss'], P.LOSS_FLOOR)
    _held('trunk', errs['trunk'], refs['trunk'], P.GRAD_FLOOR[shape])
    _held('dscale', errs['dscale'], refs['dscale'], P.LOSS_FLOOR)
    if kind != 'scalar':
        _held('lr_grad', errs['lr_grad'], refs['lr_grad'], P.LOSS_FLOOR)
    # the learner's head: exact zeros, though theta's head entries are NaN
    assert grad.size > nf and np.all(grad[nf:] == 0) and np.isfinite(grad).all() and np.isfinite(loss).all()
    # accuracy: equal on the rows whose fp64 top-2 margin is clear
    lo64 = o64['logits'][rows]
    clear = P.clear_rows(lo64)
    assert np.array_equal(logits.argmax(axis=-1)[clear], lo64.argmax(axis=-1)[clear])
    full = clear.all(axis=-1)
    assert np.array_equal(acc[full], o64['accs'][rows][full].astype(np.float32))


@pytest.mark.parametrize('case', [c for c in P.FUSED if P.FUSED[c][0] != 'min'])
def test_fused_call_against_the_fp64_oracle(case):
    """Losses (every step's) and the summed dscale and lr_grad within max(1e-4, 2 x the fp32 oracle's error), the trunk gradient within
    max(the plain ANIL call's floor, 2 x the fp32 oracle's error), accuracy equal where the fp64 margin is clear, the head's gradient 0."""
    eng = MetaEngine(_mspec(P.FUSED[case][0]))
    got = _run_case(eng, case)
    _check_vs_oracle('default', case, got)
    if case == 'omni_K0':        # no inner step: Prototypical Networks -- the merged metric head on the same inputs meets the same bars
        shape = 'omni'
        _, theta, data, labels, _, shots, nf = _inputs(shape, P.case_ids(case), head=NAN)
        ml, ma, mg, mlo = _np(*eng.meta_batch_metric(theta, data, labels, shots, 'proto', P.CASES[shape][1], return_logits=True))
        o64, o32 = _oracle(case, True), _oracle(case, False)
        l64 = o64['losses'][0]
        _held('metric loss', np.abs(ml - l64) / l64, np.abs(o32['losses'][0] - l64) / l64, P.LOSS_FLOOR)
        _held('metric trunk', rel_err(mg[:nf], o64['grad_feat']), rel_err(o32['grad_feat'], o64['grad_feat']), P.GRAD_FLOOR[shape])
        clear = P.clear_rows(o64['logits'])[0]
        assert np.array_equal(mlo.argmax(axis=-1)[clear], got[5].argmax(axis=-1)[clear]) and np.array_equal(ma[clear.all(axis=-1)], got[1][clear.all(axis=-1)])
        report('proto_anil[omni_K0][vs metric head]', loss_rel_diff=float((np.abs(ml - got[0]) / ml).max()), trunk_rel_diff=rel_err(got[2][:nf], mg[:nf]))


def test_min_against_the_fp64_oracle(conv_form):
    """The Mini-ImageNet trunk (feat 1600, the 5x5 column permutation of the step sizes' layout) under every operand form."""
    case = 'min_K2_so'
    _check_vs_oracle(conv_form, case, _run_case(MetaEngine(_mspec('min')), case))


def test_one_class_gives_loss_zero_and_zero_gradients():
    """ways = 1 through the fused call: softmax over one logit is 1, so the loss is exactly 0, the accuracy 1 and every gradient 0."""
    shots, K, T = 3, 1, 2
    eng = MetaEngine(ModelSpec.anil(1, hidden=32, channels=1, max_pool=False, in_hw=28))
    data = dev(P.synthetic.hash_uniform(7, (T, 2 * shots, 1, 28, 28)))
    labels = torch.zeros(T, 2 * shots, dtype=torch.int64, device='cuda')
    theta = dev(P.synthetic.hash_uniform(3, (eng.param_count,)) - 0.5)
    loss, acc, grad, _, dscale, _ = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, 0.125, inner_lr=0.2))
    assert np.all(loss == 0) and np.all(acc == 1) and np.all(grad == 0) and np.all(dscale == 0)


def test_evaluation_call_and_trajectory():
    """with_grad = 0: no gradient output is written, and loss / acc / logits are the bits of the call with a gradient wherever the ANIL
    call's own forward does not depend on with_grad (the ANIL call drops block 1's input Gram matrix from its evaluation call, DESIGN.md
    section 27: with the Gram route off the two calls are bit-identical; with it on, each is held to the oracle's bars above).  Row j of a
    steps call is the plain call with adapt_steps = j, row 0 is K = 0."""
    case = 'omni_K3_so_steps_scalar'
    shape, _, K, _, _, w = P.FUSED[case]
    mspec, theta, data, labels, ways, shots, nf = _inputs(shape, P.case_ids(case), head=NAN)
    T, s, lr = data.shape[0], P.CASES[shape][1], P.CASES[shape][2]
    eng = MetaEngine(mspec)
    eng.set_fused_block1(2)                     # block 1's statistics without the Gram matrix, with or without a backward half
    full = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, s, inner_lr=lr, step_w=_w(*w), return_logits=True))
    ev = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, s, inner_lr=lr, step_w=_w(*w), with_grad=False, return_logits=True))
    assert ev[2] is None and ev[3] is None and ev[4] is None
    _same('eval', ('loss', 'acc', 'logits'), (ev[0], ev[1], ev[5]), (full[0], full[1], full[5]))
    for j in range(K + 1):
        pj = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, j, s, inner_lr=lr, with_grad=False, return_logits=True))
        _same(('row', j), ('loss', 'acc', 'logits'), (ev[0][j], ev[1][j], ev[5][j]), (pj[0], pj[1], pj[5]))
    assert not np.array_equal(ev[0][0], ev[0][K])
    # the library itself: meta_grad_out stays as it was without a gradient; gradient outputs that cannot be filled are refused
    eng = MetaEngine(mspec)
    n = C.c_size_t()
    assert eng.lib.mi_anil_proto_workspace_bytes(eng._h, T, ways, shots, K, 0, 0, 0, 0, 0, C.byref(n)) == 0
    ws = eng._workspace(n.value)
    out = torch.full((eng.param_count + 3 * T,), -7.0, device='cuda')
    P_ = eng.param_count
    args = lambda wg, ds, sc=s: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), T, ways, shots, K, 1, lr, None, 0, None, sc, wg,
                                 out[P_:].data_ptr(), out[P_ + T:].data_ptr(), out.data_ptr(), None, ds, None, ws.data_ptr(), ws.numel())
    assert eng.lib.mi_meta_batch_anil_proto(*args(0, None)) == 0, eng.lib.mi_last_error(eng._h)
    torch.cuda.synchronize()
    assert bool((out[:P_] == -7.0).all()) and bool((out[P_ + 2 * T:] == -7.0).all()) and bool((out[P_:P_ + 2 * T] != -7.0).all())
    out.fill_(-7.0)
    eng.profile(True)
    for a, text in ((args(0, out[P_ + 2 * T:].data_ptr()), 'mi_meta_batch_anil_proto: dscale_out given but with_grad = 0'),
                    (args(1, None, 0.0), 'mi_meta_batch_anil_proto: scale must be positive and finite'),
                    (args(1, None, NAN), 'mi_meta_batch_anil_proto: scale must be positive and finite'),
                    (args(1, None, float('inf')), 'mi_meta_batch_anil_proto: scale must be positive and finite')):
        assert eng.lib.mi_meta_batch_anil_proto(*a) == -1 and text in eng.lib.mi_last_error(eng._h).decode(), eng.lib.mi_last_error(eng._h)
    wdev = _w(1.0)
    k0 = list(args(1, None))
    k0[8], k0[13] = 0, wdev.data_ptr()
    assert eng.lib.mi_meta_batch_anil_proto(*k0) == -1 and 'step_w needs adapt_steps >= 1, got 0' in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(T, K)
    assert eng.lib.mi_meta_batch_anil_proto(*args(1, None)) == -1
    assert 'the debug trace does not cover mi_meta_batch_anil_proto' in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(0)
    torch.cuda.synchronize()
    assert eng.profile_collect() == {} and bool((out == -7.0).all())
    eng.profile(False)
    with pytest.raises(_lib.MiError, match='positive and finite'):
        eng.meta_batch_anil_proto(theta, data, labels, shots, K, -1.0, inner_lr=lr)
    with pytest.raises(ValueError, match='exactly one of'):
        eng.meta_batch_anil_proto(theta, data, labels, shots, K, s)
    pooled = MetaEngine(ModelSpec.omniglot(ways))                       # a mean-pooled head is not an ANIL head
    with pytest.raises(_lib.MiError, match='mean-pooled'):
        pooled.meta_batch_anil_proto(torch.zeros(pooled.param_count, device='cuda'), data, labels, shots, K, s, inner_lr=lr)


# ---------------------------------------------------------------------------------------------------------------- 3: the engine
def test_graph_replay_and_another_scale():
    """Eager, capture and replays give identical bits; after theta, data and labels are overwritten IN PLACE the replayed call equals a
    fresh eager engine on the new values; another scale takes no stale graph."""
    case = 'omni_K2_so_per_step'
    shape, _, K, _, _, _ = P.FUSED[case]
    mspec, theta, data, labels, ways, shots, nf = _inputs(shape, [0, 1, 2], head=NAN)
    _, theta2, data2, labels2, _, _, _ = _inputs(shape, [3, 4, 5], head=0.5)
    theta2[:nf] *= 1.01
    vec, s = _step_args(case)['lr_vec'], P.CASES[shape][1]
    names = ('loss', 'acc', 'grad', 'lr_grad', 'dscale', 'logits')
    call = lambda e, th, d, l, sc: _np(*e.meta_batch_anil_proto(th, d, l, shots, K, sc, lr_vec=vec, want_lr_grad=True, return_logits=True))
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    first = call(eng, theta, data, labels, s)
    for i in range(2):
        _same(('replay', i), names, call(eng, theta, data, labels, s), first)
    _same('eager', names, call(MetaEngine(mspec), theta, data, labels, s), first)
    other = call(eng, theta, data, labels, 2 * s)
    _same('scale', names, other, call(MetaEngine(mspec), theta, data, labels, 2 * s))
    assert not np.array_equal(other[0], first[0]) and not np.array_equal(other[2], first[2])
    theta.copy_(theta2); data.copy_(data2); labels.copy_(labels2)
    replayed = call(eng, theta, data, labels, s)
    _same('in_place', names, replayed, call(MetaEngine(mspec), theta2, data2, labels2, s))
    assert not np.array_equal(replayed[0], first[0])
    eng.set_graph(False)


def test_launch_make_up():
    """The launches of mi_meta_batch_anil_lr / _steps on the same arguments, plus exactly one proto_init/0 and, with a gradient, one
    proto_init/1 -- at T = 1 and T = 3, first and second order, with and without lr_grad."""
    shape, K = 'omni', 2
    s, lr = P.CASES[shape][1], P.CASES[shape][2]
    for ids in ([0], [0, 1, 2]):
        mspec, theta, data, labels, ways, shots, _ = _inputs(shape, ids, head=0.25)
        eng = MetaEngine(mspec)
        vec, w = dev(P.lr_vector(128, ways, lr, K, 5)), _w(0.3, 0.7)
        for fo in (False, True):
            for wg in (True, False):
                pairs = {
                    'lr': (lambda: eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec, first_order=fo, with_grad=wg, want_lr_grad=wg),
                           lambda: eng.meta_batch_anil_proto(theta, data, labels, shots, K, s, lr_vec=vec, first_order=fo, with_grad=wg, want_lr_grad=wg)),
                    'steps': (lambda: eng.meta_batch_anil_steps(theta, data, labels, shots, K, w, inner_lr=lr, first_order=fo, with_grad=wg),
                              lambda: eng.meta_batch_anil_proto(theta, data, labels, shots, K, s, inner_lr=lr, step_w=w, first_order=fo, with_grad=wg)),
                }
                for name, (plain, proto) in pairs.items():
                    base, got = _census(eng, plain), _census(eng, proto)
                    assert got.pop('proto_init/0') == 1 and got.pop('proto_init/1', 0) == (1 if wg else 0), (ids, fo, wg, name, got)
                    assert got == base and 'proto_init/0' not in base, (ids, fo, wg, name, got, base)


# ---------------------------------------------------------------------------------------------------------------- 4: Python
def _learner(shape, lr):
    """(features, MAML head, Linear) with the fixtures' trunk; lr: a number, or a function head -> InnerLR."""
    _, _, _, fc, ways, _ = P.SHAPES[shape]
    features = _trunk(shape)
    head = torch.nn.Linear(fc, ways).cuda()
    return features, cf.MAML(head, lr=lr(head) if callable(lr) else lr), head


def test_backward_fills_trunk_scale_and_step_size_gradients():
    """.backward() leaves the engine call's bits in the trunk's .grad, the chain rule dscale_sum * scale in init.log_scale.grad, the
    per-tensor sums of lr_grad in a learnable InnerLR's values.grad and zeros in the learner's weight and bias; under no_grad the call only
    scores; fast_adapt_proto_anil is the T = 1 view."""
    shape, K = 'omni', 2
    mspec, theta, data, labels, ways, shots, nf = _inputs(shape, head=0.0)
    s = P.CASES[shape][1]
    make = lambda head: cf.InnerLR(head, torch.tensor([[0.2, 0.1], [0.15, 0.25]]), per='tensor', steps=K, learnable=True)
    features, maml, head = _learner(shape, make)
    theta[nf:] = torch.cat([head.weight.detach().reshape(-1), head.bias.detach()])
    init = cf.ProtoInit(s).cuda()
    params = list(features.parameters())
    eng = MetaEngine(mspec)
    flat = maml.lr.flat().detach().contiguous()
    w = (0.3, 0.7)
    objective, losses, accs = cf.meta_batch_adapt_proto_anil(maml.clone(), features, init, data, labels, K, shots, ways, step_weights=list(w))
    assert tuple(losses.shape) == tuple(accs.shape) == (K + 1, data.shape[0]) and not losses.requires_grad
    objective.backward()
    l, a, g, lg, ds, _ = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, init.scale, lr_vec=flat, step_w=_w(*w), want_lr_grad=True))
    assert np.array_equal(_grads(params), g[:nf]) and np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a)
    assert bool((head.weight.grad == 0).all()) and bool((head.bias.grad == 0).all())
    want = np.float32(ds.astype(np.float64).sum() * init.scale)
    assert init.log_scale.grad.item() == want and want != 0
    twin = make(head)
    (twin.flat() * torch.from_numpy(lg).cuda()).sum().backward()
    assert np.array_equal(maml.lr.values.grad.cpu().numpy(), twin.values.grad.cpu().numpy()) and np.abs(lg).sum() > 0
    # the plain objective, a scalar step, a fixed scale
    for p in params + [init.log_scale, head.weight, head.bias]:
        p.grad = None
    fixed = cf.ProtoInit(s, learnable=False).cuda()
    plain = cf.MAML(head, lr=0.2)
    total, losses, accs = cf.meta_batch_adapt_proto_anil(plain.clone(), features, fixed, data, labels, K, shots, ways)
    total.backward()
    l, a, g, _, _, _ = _np(*eng.meta_batch_anil_proto(theta, data, labels, shots, K, fixed.scale, inner_lr=0.2))
    assert tuple(losses.shape) == (data.shape[0],) and np.array_equal(_grads(params), g[:nf]) and np.array_equal(_np(losses)[0], l)
    assert total.item() == pytest.approx(float(l.sum()), rel=1e-6)
    with torch.no_grad():
        total, losses2, _ = cf.meta_batch_adapt_proto_anil(plain.clone(), features, fixed, data, labels, K, shots, ways)
    assert not total.requires_grad and np.allclose(_np(losses2)[0], l, rtol=2e-4)
    with pytest.raises(RuntimeError):
        total.backward()
    for p in params:
        p.grad = None
    loss, acc = cf.fast_adapt_proto_anil((data[0].cpu(), labels[0].cpu()), plain.clone(), features, fixed, K, shots, ways, torch.device('cuda'))
    loss.backward()
    l1, a1, g1, _, _, _ = _np(*eng.meta_batch_anil_proto(theta, data[:1].contiguous(), labels[:1].contiguous(), shots, K, fixed.scale, inner_lr=0.2))
    assert loss.item() == l1[0] and acc.item() == a1[0] and np.array_equal(_grads(params), g1[:nf])


def test_evaluate_step_zero_is_prototypical_networks():
    """evaluate_proto_anil returns the K + 1 mean accuracies of one call; step 0 equals fast_adapt_metric(..., 'proto', s) on the same tasks."""
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    shape, K = 'omni', 2
    dataset, _, _, _, ways, shots = P.SHAPES[shape]
    s = P.CASES[shape][1]
    features, maml, _ = _learner(shape, 0.2)
    init = cf.ProtoInit(s, learnable=False).cuda()

    class Tasks(SyntheticTasks):
        def sample(self):
            d, l = super().sample()
            return d.view(-1, 1, 28, 28), l
    p = dict(meta_batch_size=3, adapt_steps=K, shots=shots, ways=ways)
    per_step = cf.evaluate_proto_anil(p, Tasks(dataset, ways, shots, 0), maml, features, init, torch.device('cuda'))
    assert isinstance(per_step, list) and len(per_step) == K + 1 and all(0.0 <= a <= 1.0 for a in per_step)
    tasks = Tasks(dataset, ways, shots, 0)
    with torch.no_grad():
        accs = [cf.fast_adapt_metric(tasks.sample(), features, shots, ways, torch.device('cuda'), metric='proto', scale=s)[1].item() for _ in range(3)]
    assert per_step[0] == pytest.approx(float(np.mean(accs)), abs=1e-6)
    assert cf.evaluate_proto_anil(dict(p, adapt_steps=0), Tasks(dataset, ways, shots, 0), maml, features, init, torch.device('cuda')) == \
        pytest.approx(per_step[:1], abs=1e-6)


def test_driver_with_and_without_the_flag(tmp_path):
    """Two iterations of vision.anil_vision with --proto_init move the trunk and the scale, leave the learner's head where it was, save
    proto_init.pt beside head.pt and reload; without the flag the driver's output keys are what they were."""
    from exploring_meta_amd.vision import anil_vision
    common = ['--dataset', 'omni', '--shots', '1', '--adapt_steps', '2', '--meta_batch_size', '3', '--num_iterations', '2', '--inner_lr', '0.2']
    logs = []
    (features, head, init), metrics = anil_vision.main(common + ['--proto_init', '--proto_scale', '0.125', '--multi_step_loss', '--msl_iterations',
                                                                 '1', '--save_dir', str(tmp_path)], log=logs.append)
    assert len(logs) == 2 and all(math.isfinite(v) for v in metrics.values())
    assert set(metrics) == {'train_loss', 'train_acc', 'valid_loss', 'valid_acc', 'proto_scale'}
    assert isinstance(init, cf.ProtoInit) and init.scale != 0.125 and metrics['proto_scale'] == init.scale
    # (checkpoints: model_*_1.pt after the first step, *.pt after the second)
    load = lambda *parts: torch.load(os.path.join(tmp_path, *parts))
    first, last = load('model_checkpoints', 'model_features_1.pt'), load('features.pt')
    assert any(not torch.equal(first[k], last[k]) for k in first if first[k].is_floating_point())
    first, last = load('model_checkpoints', 'model_head_1.pt'), load('head.pt')
    assert set(first) == set(last) and all(torch.equal(first[k], last[k]) for k in first)          # zero gradients: Adam leaves the head alone
    assert bool((head.module.weight.grad == 0).all()) and bool((head.module.bias.grad == 0).all())
    for name in ('features.pt', 'head.pt', 'proto_init.pt'):
        assert os.path.exists(tmp_path / name), name
    again = cf.ProtoInit()
    again.load_state_dict(torch.load(tmp_path / 'proto_init.pt'))
    assert again.scale == init.scale
    result, metrics = anil_vision.main(common, log=logs.append)
    assert len(result) == 2 and set(metrics) == {'train_loss', 'train_acc', 'valid_loss', 'valid_acc'}
