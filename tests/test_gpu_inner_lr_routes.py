"""The step-size-vector MAML call (mi_meta_batch_maml_lr) on the routes tests/test_gpu_inner_lr.py does not reach: the separate launches
of set_fused_tail(0) (axpy_vec / scale_vec / product of misc.hip), train + validation tasks in one call (grad_tasks < T), K = 3 (the
third swap of the direction buffers), block 1 by conv-recompute and by the generic kernels, 5-shot, adapt_steps = 0, step sizes of both
signs and all zero, and graph replay with and without lr_grad.  Bit identity between routes that run the same arithmetic, the call's own
trace element by element, and the fp64 oracle (tests/inner_lr_oracle.py) by the rule of test_gpu_inner_lr.py::_held.
Shapes: Mini-ImageNet net 5-way 1-shot tasks 0..4 with K <= 3 and 5-shot task 0 with K = 2, Omniglot net 5-way 1-shot tasks 0, 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd.engine import MetaEngine
from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from helpers import model_params, task_tensors
from gpu_utils import rel_err, report
import inner_lr_oracle as O
from test_gpu_inner_lr import _held, _np, _oracle as _oracle_k2, _specs, _steps

pytestmark = pytest.mark.gpu

WAYS = 5
LOSS_FLOOR, GRAD_FLOOR = 1e-4, 2e-3     # test_gpu_engine.py::CASES: Mini-ImageNet 1-shot and 5-shot at K >= 2 (K = 3 takes the K = 2 row)
NAMES = ('loss', 'acc', 'grad', 'lr_grad', 'logits')
TRACED = ('theta', 'g', 'lam_in', 'hv')


def _inputs(net, tasks, shots=1):
    spec, mspec = _specs(net)
    theta = R.flatten_params(model_params(spec, 11)).float().cuda().contiguous()
    data, labels = synthetic.make_meta_batch(net, tasks, WAYS, shots)
    return mspec, theta, torch.from_numpy(data).cuda().contiguous(), torch.from_numpy(labels).cuda().contiguous()


def _mixed(net, K, base=0.4, seed=5):
    """One vector per step, non-uniform, block 1 frozen, a quarter of the other entries negative."""
    return O.lr_vector(_specs(net)[0], base, K, seed, negative=0.25)


def _call(eng, theta, data, labels, shots, K, vec, **kw):
    kw.setdefault('want_lr_grad', True)
    return _np(*eng.meta_batch_lr(theta, data, labels, shots, K, vec, return_logits=True, **kw))


def _traced(eng, T, K, fn):
    """fn()'s outputs followed by the four traced arrays of that call."""
    tr = eng.set_trace(T, K)
    out = fn()
    out = out + _np(*(tr[k] for k in TRACED))
    eng.set_trace(0)
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('net,K,fo,fused1', [('min', 3, False, 1), ('min', 2, False, 2), ('min', 2, False, 0), ('omni', 2, False, 1),
                                             ('min', 2, True, 1)])
def test_vector_call_fused_tail_is_bit_identical(net, K, fo, fused1):
    """test_gpu_engine.py::test_fused_tail_is_bit_identical for the vector call, with one vector per step of both signs and lr_grad: the
    one-launch advance (gram.hip advance_kernel<true>: a - lr[e] * g, dir = lr[e] * lam, prod = g * lam) against axpy_vec / scale_vec /
    product of misc.hip -- a separate multiply and subtract per element on both sides, so every output and every traced vector has the
    same bits.  K = 3 is the first call that writes a direction buffer a second time."""
    tasks = [0, 1, 2] if net == 'min' else [0, 1]
    mspec, theta, data, labels = _inputs(net, tasks)
    vec = torch.from_numpy(_mixed(net, K)).cuda()
    outs = []
    for on in (1, 0, 1):
        eng = MetaEngine(mspec)
        eng.set_fused_block1(fused1)
        eng.set_fused_tail(on)
        run = lambda: _call(eng, theta, data, labels, 1, K, vec, first_order=fo)
        outs.append(run() if fo else _traced(eng, len(tasks), K, run))
    for o in outs[1:]:
        assert len(o) == len(outs[0]) == (5 if fo else 9)
        for name, a, b in zip(NAMES + TRACED, o, outs[0]):
            assert np.array_equal(a, b), (name, rel_err(a, b))
    for i in (2, 3):
        assert np.isfinite(outs[0][i]).all() and np.abs(outs[0][i]).sum() > 0
    assert outs[0][3].shape == (K, theta.numel())


@pytest.mark.parametrize('fused1', [1, 2])
def test_vector_call_fused_finalize_is_bit_identical(fused1):
    """test_gpu_engine.py::test_fused_finalize_is_bit_identical for the vector call at K = 2 (Gram-matrix block 1, and conv-recompute block 1
    whose tangent statistics are the partials of the pass driven with D lam): the fold order is the same, so are the bits."""
    net, K, tasks = 'min', 2, [0, 1, 2]
    mspec, theta, data, labels = _inputs(net, tasks)
    vec = torch.from_numpy(_mixed(net, K)).cuda()
    outs = []
    for on in (1, 0, 1):
        eng = MetaEngine(mspec)
        eng.set_fused_block1(fused1)
        eng.set_fused_finalize(on)
        outs.append(_traced(eng, len(tasks), K, lambda: _call(eng, theta, data, labels, 1, K, vec)))
    for o in outs[1:]:
        for name, a, b in zip(NAMES + TRACED, o, outs[0]):
            assert np.array_equal(a, b), (name, rel_err(a, b))
    assert np.isfinite(outs[0][3]).all() and np.abs(outs[0][3]).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 2
def test_separate_launches_lr_grad_is_the_fold_and_the_updates_are_exact():
    """set_fused_tail(0), K = 3, one vector per step of both signs -- the twin of test_gpu_inner_lr.py::
    test_lr_grad_is_the_fold_of_the_traced_vectors with its derived bound (n + 2) 2^-24 sum |g lam| + n 2^-126, n = T terms per step.
    And from the same trace, in exact fp32 (one rounding of the product, one of the difference, as the kernels state):
    theta[k+1] == theta[k] - lr[k] * g[k] (axpy_vec), lam_in[k-1] == lam_in[k] - hv[k] (the adjoint update with alpha = 1), and the
    meta-gradient == the task-ordered fp32 sum of lam_in[0] - hv[0]."""
    net, K, tasks = 'min', 3, [0, 1, 2]
    mspec, theta, data, labels = _inputs(net, tasks)
    T = len(tasks)
    lr = _mixed(net, K)
    eng = MetaEngine(mspec)
    eng.set_fused_tail(0)
    _, _, grad, lr_grad, _, th, g, lam, hv = _traced(eng, T, K, lambda: _call(eng, theta, data, labels, 1, K, torch.from_numpy(lr).cuda()))
    assert all(np.isfinite(x).all() for x in (grad, lr_grad, th, g, lam, hv))
    prod = g.astype(np.float64) * lam.astype(np.float64)                      # [K, T, P]
    want, mag = -prod.sum(1), np.abs(prod).sum(1)
    bound = (T + 2) * 2.0 ** -24 * mag + T * 2.0 ** -126
    excess = np.abs(lr_grad - want) - bound
    report('inner_lr_routes_trace[tail0 K3]', worst_excess=float(excess.max()), rel=rel_err(lr_grad, want))
    assert lr_grad.shape == (K, theta.numel()) and np.all(excess <= 0)
    assert (lr < 0).any() and (lr > 0).any()
    for k in range(K):
        step = (lr[k][None] * g[k]).astype(np.float32)                          # fp32 product, rounded, then the fp32 difference
        assert step.dtype == np.float32 and np.array_equal(th[k + 1], th[k] - step), k
        moved = lr[k] != 0
        assert not np.array_equal(th[k + 1][:, moved], th[k][:, moved])
    for k in range(1, K):
        assert np.array_equal(lam[k - 1], lam[k] - hv[k]), k
        assert np.abs(hv[k]).sum() > 0
    lam0 = lam[0] - hv[0]
    total = np.zeros_like(lam0[0])
    for t in range(T):
        total = total + lam0[t]
    assert np.array_equal(grad, total)


# ---------------------------------------------------------------------------------------------------------------- 3
@functools.lru_cache(maxsize=None)
def _oracle(tasks, shots, K, base, negative, fp64):
    """One oracle run per case and precision (Mini-ImageNet net, second order, one vector per step, seed 5), shared and never modified."""
    spec, _ = _specs('min')
    dtype = torch.float64 if fp64 else torch.float32
    datas, labels = task_tensors('min', list(tasks), WAYS, shots, dtype)
    lr = O.lr_vector(spec, base, K, 5, negative=negative)
    return O.meta_batch(model_params(spec, 11), spec, datas, labels, K, shots, WAYS, lr, False, dtype)


def _hold_to_oracle(tag, got, o64, o32, n_grad=None):
    """Loss, meta-gradient and lr_grad within max(floor, 2 x the fp32 oracle's own error), accuracy / argmax where the fp64 top-2 margin is
    clear (test_gpu_inner_lr.py::test_vector_call_vs_fp64_oracle).  o64 / o32: (losses, accs, grad, lr_grad, logits) of the oracle."""
    loss, acc, grad, lr_grad, logits = got
    l64, a64, g64, lg64, lo64 = o64
    l32, _, g32, lg32, _ = o32
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), grad=rel_err(grad, g64), lr_grad=rel_err(lr_grad, lg64))
    refs = dict(loss=np.abs(l32 - l64) / np.abs(l64), grad=rel_err(g32, g64), lr_grad=rel_err(lg32, lg64))
    report(f'inner_lr_routes_oracle[{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           grad_rel_err=errs['grad'], ref_fp32_grad_rel_err=refs['grad'], lr_grad_rel_err=errs['lr_grad'],
           ref_fp32_lr_grad_rel_err=refs['lr_grad'])
    _held('loss', errs['loss'], refs['loss'], LOSS_FLOOR)
    _held('grad', errs['grad'], refs['grad'], GRAD_FLOOR)
    _held('lr_grad', errs['lr_grad'], refs['lr_grad'], GRAD_FLOOR)
    assert lr_grad.shape == lg64.shape and len(lo64) == len(loss)
    for t in range(len(lo64)):
        top2 = np.sort(lo64[t], axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * max(1.0, np.abs(lo64[t]).max())
        assert np.array_equal(logits[t].argmax(axis=1)[clear], lo64[t].argmax(axis=1)[clear])
        if clear.all():
            assert acc[t] == a64[t]


def test_three_steps_vs_fp64_oracle(conv_form):
    """Case a: K = 3, one vector per step (0.4 * U(0.5, 1.5), block 1 frozen), tasks 0, 1, on every operand form -- the direction buffers
    swap three times.
    Measured (engine / fp32 oracle, from fp64): loss 5e-8 .. 4.1e-7 / 2.3e-7, meta-gradient 5.1e-5 .. 6.8e-5 / 5.1e-5, lr_grad 3.19e-4 ..
    3.24e-4 / 3.19e-4 over the four forms."""
    tasks, K = (0, 1), 3
    mspec, theta, data, labels = _inputs('min', list(tasks))
    vec = torch.from_numpy(O.lr_vector(_specs('min')[0], 0.4, K, 5)).cuda()
    got = _call(MetaEngine(mspec), theta, data, labels, 1, K, vec)
    _hold_to_oracle(f'a K3][{conv_form}', got, _oracle(tasks, 1, K, 0.4, 0.0, True)[:5], _oracle(tasks, 1, K, 0.4, 0.0, False)[:5])


def test_mixed_sign_steps_vs_fp64_oracle():
    """Case b: K = 2, a quarter of the non-frozen step sizes negative (a learnt step size can cross zero), tasks 1, 2.
    (Not tasks 0, 1: with these signs a pooling decision of task 0 is near a tie and falls the other way on the split-bf16 form alone --
    task 0 by itself: meta-gradient 1.6e-3 / lr_grad 3.2e-3 from fp64 there, while the fp32 pipe, the split-fp16 form and the fp32 oracle
    all sit at 3.1e-5 / 3.8e-4.  On tasks 1, 2 the fp32 oracle is within 1e-5 of fp64, far inside half the floors.)
    Measured (engine / fp32 oracle): loss 5.6e-7 / 1.3e-7, meta-gradient 4.6e-6 / 2.1e-6, lr_grad 4.3e-6 / 5.4e-6."""
    tasks, K = (1, 2), 2
    mspec, theta, data, labels = _inputs('min', list(tasks))
    lr = _mixed('min', K)
    assert (lr < 0).any()
    got = _call(MetaEngine(mspec), theta, data, labels, 1, K, torch.from_numpy(lr).cuda())
    _hold_to_oracle('b mixed signs', got, _oracle(tasks, 1, K, 0.4, 0.25, True)[:5], _oracle(tasks, 1, K, 0.4, 0.25, False)[:5])


def test_five_shot_vs_fp64_oracle():
    """Case c: 5-shot (25 rows per pass), K = 2, one vector per step with base 0.1, task 0.
    Measured (engine / fp32 oracle): loss 3.1e-7 / 5.5e-7, meta-gradient 1.1e-6 / 6.3e-5, lr_grad 1.2e-6 / 2.9e-4."""
    tasks, K, shots = (0,), 2, 5
    mspec, theta, data, labels = _inputs('min', list(tasks), shots)
    vec = torch.from_numpy(O.lr_vector(_specs('min')[0], 0.1, K, 5)).cuda()
    got = _call(MetaEngine(mspec), theta, data, labels, shots, K, vec)
    _hold_to_oracle('c 5-shot', got, _oracle(tasks, shots, K, 0.1, 0.0, True)[:5], _oracle(tasks, shots, K, 0.1, 0.0, False)[:5])


def _per_task_lr_grad(g, lam):
    """lr_steps == K: task t's share of row k of lr_grad is -g[k][t] * lam_in[k][t]  ->  [T, K, P]."""
    return -(g.astype(np.float64) * lam.astype(np.float64)).transpose(1, 0, 2)


@pytest.mark.parametrize('fused1', [2, 0])
def test_block1_recompute_and_generic_routes_vs_fp64_oracle(fused1):
    """Case d: block 1 by the conv-recompute kernels (2) and by the generic kernels (0), K = 2, tasks 1..3 -- the Hessian-vector pass is driven
    with D lam and block 1's tangent statistics come from that direction.  Against the oracle by the rule, and each task's lr_grad (from the
    trace) against the default route by the per-task bar of test_gpu_engine.py::test_fused_block1_matches_generic_kernels.
    (Not tasks 0..2: task 0 carries a near-tied pooling decision -- its fp32 oracle is 2.5e-4 / 4.3e-4 from fp64 where the other tasks' is
    1e-5 -- that the conv-recompute route takes the other way: that task's lr_grad 5.1e-3 from the default route, tasks 1, 2 at 2.5e-6 and
    9.4e-6, the call still within the oracle rule at 1.0e-3 / 1.7e-3.  On tasks 1..3 each task's fp32 oracle is within 2.2e-4 of fp64.)
    Measured (engine / fp32 oracle): conv-recompute loss 1.2e-6 / 5.1e-7, meta-gradient 5.1e-6 / 6.0e-5, lr_grad 5.6e-6 / 1.4e-4, per task against
    the default route 2.5e-6, 9.4e-6, 6.4e-6; generic kernels 6.4e-7, 5.2e-6, 5.4e-6 and 3.0e-6, 8.7e-6, 4.5e-6."""
    K, tasks = 2, [1, 2, 3]
    mspec, theta, data, labels = _inputs('min', tasks)
    vec = torch.from_numpy(_steps('min', K, True)).cuda()
    outs = {}
    for f in (1, fused1):
        eng = MetaEngine(mspec)
        eng.set_fused_block1(f)
        outs[f] = _traced(eng, len(tasks), K, lambda: _call(eng, theta, data, labels, 1, K, vec))
    _hold_to_oracle(f'd fused_block1 {fused1}', outs[fused1][:5], _oracle(tuple(tasks), 1, K, 0.4, 0.0, True)[:5],
                    _oracle(tuple(tasks), 1, K, 0.4, 0.0, False)[:5])
    mine, base = _per_task_lr_grad(outs[fused1][6], outs[fused1][7]), _per_task_lr_grad(outs[1][6], outs[1][7])
    errs = [rel_err(mine[t], base[t]) for t in range(len(tasks))]
    report(f'inner_lr_routes_block1[{fused1}]', lr_grad_rel_per_task=errs)
    assert sorted(errs)[1] < 1e-4 and max(errs) < 5e-3, errs
    assert rel_err(mine.sum(0), outs[fused1][3]) < 1e-6                          # the per-task shares are the shares of the call's lr_grad


@pytest.mark.parametrize('fused_tail', [1, 0])
def test_train_and_validation_in_one_vector_call(fused_tail):
    """Case e: 3 train + 2 validation tasks (the call vision/maml_vision.py makes every iteration), K = 2, on the one-launch advance and
    on the separate launches.  Oracle: the train tasks for the meta-gradient and lr_grad, all five for loss / accuracy / logits.  And
    against the two separate calls with the bars of test_gpu_engine.py::test_train_and_validation_tasks_in_one_call (loss, logits 2e-4;
    gradients 2e-3 at K = 2); grad_tasks = T is the plain call bit for bit.
    Measured, the same on both routes (engine / fp32 oracle): loss 1.0e-6 / 6.6e-7, meta-gradient 9.1e-5 / 1.1e-4, lr_grad 1.4e-4 / 2.1e-4; the one
    call and the two separate calls came out with the same bits."""
    K, tasks, G = 2, [0, 1, 2, 3, 4], 3
    mspec, theta, d, l = _inputs('min', tasks)
    vec = torch.from_numpy(_steps('min', K, True)).cuda()
    eng = MetaEngine(mspec)
    eng.set_fused_tail(fused_tail)
    got = _call(eng, theta, d, l, 1, K, vec, grad_tasks=G)
    both = []
    for fp64 in (True, False):
        tr, va = _oracle_k2('min', K, True, False, fp64), _oracle((3, 4), 1, K, 0.4, 0.0, fp64)
        both.append((np.concatenate([tr[0], va[0]]), np.concatenate([tr[1], va[1]]), tr[2], tr[3], list(tr[4]) + list(va[4])))
    _hold_to_oracle(f'e grad_tasks 3 of 5 tail{fused_tail}', got, both[0], both[1])
    train = _call(eng, theta, d[:G], l[:G], 1, K, vec)
    valid = _call(eng, theta, d[G:], l[G:], 1, K, vec, grad_tasks=0, want_lr_grad=False)
    assert valid[2] is None and valid[3] is None
    want_l, want_a, want_lo = (np.concatenate([train[i], valid[i]]) for i in (0, 1, 4))
    e_l = float((np.abs(got[0] - want_l) / np.abs(want_l)).max())
    e_lo, e_g, e_lg = rel_err(got[4], want_lo), rel_err(got[2], train[2]), rel_err(got[3], train[3])
    report(f'inner_lr_routes_train_valid[tail{fused_tail}]', loss_rel=e_l, logits_rel=e_lo, grad_rel=e_g, lr_grad_rel=e_lg)
    assert e_l < 2e-4 and e_lo < 2e-4 and e_g < 2e-3 and e_lg < 2e-3 and np.array_equal(got[1], want_a)
    for a, b in zip(_call(eng, theta, d, l, 1, K, vec, grad_tasks=len(tasks)), _call(eng, theta, d, l, 1, K, vec)):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_no_inner_steps():
    """adapt_steps = 0 with a [1, P] or [P] vector and lr_grad: the scalar call's bits at K = 0, lr_grad exactly zero.  Vectors that
    are no [1, P] are refused before any launch, by the wrapper and by the library."""
    mspec, theta, data, labels = _inputs('min', [0, 1, 2])
    eng = MetaEngine(mspec)
    P = eng.param_count
    want = _np(*eng.meta_batch(theta, data, labels, 1, 0, 0.4, return_logits=True))
    row = _mixed('min', 1)
    for vec in (row, row[0]):
        loss, acc, grad, lr_grad, logits = _call(eng, theta, data, labels, 1, 0, torch.from_numpy(vec).cuda().contiguous())
        for name, a, b in zip(('loss', 'acc', 'grad', 'logits'), (loss, acc, grad, logits), want):
            assert np.array_equal(a, b), name
        assert lr_grad.shape == (1, P) and not lr_grad.any()
    assert np.abs(want[2]).sum() > 0
    eng.profile(True)
    ok = torch.from_numpy(row).cuda()
    with pytest.raises(_lib.MiError, match='lr_vec has shape'):
        eng.meta_batch_lr(theta, data, labels, 1, 0, ok[:0].contiguous(), want_lr_grad=True)
    with pytest.raises(_lib.MiError, match='lr_steps = 2 must be 1 or adapt_steps = 0'):
        eng.meta_batch_lr(theta, data, labels, 1, 0, torch.cat([ok, ok]).contiguous(), want_lr_grad=True)
    ws = eng._workspace(eng.workspace_bytes(3, 1, 2, True) + (1 << 20))
    out = torch.empty(2 * P + 6, device='cuda')
    args = lambda K, steps: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), 3, 3, WAYS, 1, K, ok.data_ptr(), steps, 1,
                             out[2 * P:].data_ptr(), out[2 * P + 3:].data_ptr(), out.data_ptr(), out[P:].data_ptr(), None, ws.data_ptr(), ws.numel())
    for K, steps, text in ((0, 0, 'lr_steps = 0 must be 1 or adapt_steps = 0 (without inner steps: 1)'),
                           (0, 2, 'lr_steps = 2 must be 1 or adapt_steps = 0 (without inner steps: 1)'),
                           (2, 0, 'lr_steps = 0 must be 1 or adapt_steps = 2'), (2, -1, 'lr_steps = -1 must be 1 or adapt_steps = 2')):
        assert eng.lib.mi_meta_batch_maml_lr(*args(K, steps)) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode()
    b = C.c_size_t()
    assert eng.lib.mi_workspace_bytes_lr(eng._h, 3, WAYS, 1, 0, 1, 0, 1, C.byref(b)) != 0
    assert eng.profile_collect() == {}
    eng.profile(False)


def test_one_step_vector_shapes_give_the_same_bits():
    """lr_steps = K = 1: [1, P] and [P] are the same call."""
    mspec, theta, data, labels = _inputs('min', [0, 1, 2])
    eng = MetaEngine(mspec)
    row = _mixed('min', 1, base=0.5)
    a = _call(eng, theta, data, labels, 1, 1, torch.from_numpy(row).cuda())
    b = _call(eng, theta, data, labels, 1, 1, torch.from_numpy(row[0].copy()).cuda())
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and np.array_equal(x, y), name
    assert a[3].shape == (1, eng.param_count) and np.abs(a[3]).sum() > 0


@pytest.mark.parametrize('fused1', [1, 2, 0])
def test_all_step_sizes_zero(fused1):
    """Nothing adapts: theta_K == theta_0 bitwise in the trace, every Hessian-vector product (driven with the zero vector) is zero, the
    support gradients of the steps are the same bits, and lr_grad -- how the query loss would change if a step size left zero -- is not
    zero.  Loss, accuracy, logits and the meta-gradient, second order and first order, are the bits of the scalar call with step 0, and
    the bits of the K = 0 call (the query gradient at theta_0) where block 1 runs by conv-recompute (2) or by the generic kernels (0).
    On the default route (1) the K = 0 call is NOT the same arithmetic: make_plan (engine.hip) takes block 1's statistics from the input
    Gram matrix only when the support set is swept at least twice, so the query pass of a K = 2 call has Gram-matrix statistics and that
    of a K = 0 call has not (measured: loss 1.7e-7, logits 8.4e-7, meta-gradient 9.5e-7 apart).  There the K = 0 call is held with the
    bars of test_gpu_engine.py::test_fused_block1_matches_generic_kernels for loss, accuracy and logits -- the same two ways of rounding
    block 1 -- and the meta-gradient with that file's bar without inner-loop amplification, 1e-4."""
    K, tasks = 2, [0, 1, 2]
    mspec, theta, data, labels = _inputs('min', tasks)
    eng = MetaEngine(mspec)
    eng.set_fused_block1(fused1)
    zeros = torch.zeros(K, eng.param_count, device='cuda')
    got = _traced(eng, len(tasks), K, lambda: _call(eng, theta, data, labels, 1, K, zeros))
    th, g, lam, hv = got[5:]
    for k in range(1, K + 1):
        assert np.array_equal(th[k], th[0])
    assert np.array_equal(th[0], np.broadcast_to(theta.cpu().numpy(), th[0].shape))
    assert not hv.any() and np.array_equal(g[1], g[0]) and np.array_equal(lam[1], lam[0])
    k0 = _np(*eng.meta_batch(theta, data, labels, 1, 0, 0.4, return_logits=True))
    for fo in (False, True):
        out = got if not fo else _call(eng, theta, data, labels, 1, K, zeros, first_order=True)
        out = (out[0], out[1], out[2], out[4], out[3])
        scalar = _np(*eng.meta_batch(theta, data, labels, 1, K, 0.0, first_order=fo, return_logits=True))
        for name, a, b, c in zip(('loss', 'acc', 'grad', 'logits'), out, scalar, k0):
            assert np.array_equal(a, b), (fo, name, rel_err(a, b))
            if fused1 != 1:
                assert np.array_equal(a, c), (fo, name, rel_err(a, c))
        report(f'inner_lr_routes_zero_steps[fused_block1 {fused1} fo{int(fo)}]', loss_rel=rel_err(out[0], k0[0]), grad_rel=rel_err(out[2], k0[2]),
               logits_rel=rel_err(out[3], k0[3]))
        assert np.allclose(out[0], k0[0], rtol=1e-5) and np.array_equal(out[1], k0[1])
        assert np.allclose(out[3], k0[3], rtol=1e-4, atol=1e-4) and rel_err(out[2], k0[2]) < 1e-4
        lr_grad = out[4]
        assert lr_grad.shape == (K, eng.param_count) and np.isfinite(lr_grad).all() and np.abs(lr_grad).sum() > 0
        if fo:                                                    # first order: both rows are -sum_t g_0 * grad L_query(theta_0)
            assert np.array_equal(lr_grad[0], lr_grad[1])


def test_graph_replay_with_and_without_lr_grad():
    """set_graph(True), the same buffers, want_lr_grad alternating True / False / True ... (two cached graphs: with and without the
    products and the fold), all tasks train tasks and 3 of 5: the eager bits every time, through eager run, capture and replays; after the
    step sizes are overwritten in place the replayed lr_grad in the persistent buffer is that of the new values, not the old one."""
    K = 2
    mspec, theta, data, labels = _inputs('min', [0, 1, 2, 3, 4])
    lr_a, lr_b = _mixed('min', K), O.lr_vector(_specs('min')[0], 0.3, K, 9, frozen=('linear.',), negative=0.25)
    fresh = MetaEngine(mspec)
    fresh.set_graph(False)
    for gt in (3, None):
        ref = {(tag, want): _call(fresh, theta, data, labels, 1, K, torch.from_numpy(v).cuda(), grad_tasks=gt, want_lr_grad=want)
               for tag, v in (('a', lr_a), ('b', lr_b)) for want in (True, False)}
        eng = MetaEngine(mspec)
        eng.set_graph(True)
        vec = torch.from_numpy(lr_a).cuda()
        for i in range(8):                                                   # each of the two signatures: eager, capture, replay, replay
            want = i % 2 == 0
            out = _call(eng, theta, data, labels, 1, K, vec, grad_tasks=gt, want_lr_grad=want)
            assert (out[3] is not None) == want
            for name, a, b in zip(NAMES, out, ref['a', want]):
                assert (a is None and b is None) or np.array_equal(a, b), (gt, i, name)
        vec.copy_(torch.from_numpy(lr_b))
        for want in (True, False, True):
            out = _call(eng, theta, data, labels, 1, K, vec, grad_tasks=gt, want_lr_grad=want)
            for name, a, b in zip(NAMES, out, ref['b', want]):
                assert (a is None and b is None) or np.array_equal(a, b), (gt, want, name)
        assert not np.array_equal(ref['a', True][3], ref['b', True][3])
