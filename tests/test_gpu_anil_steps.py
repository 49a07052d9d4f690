"""Per-parameter step sizes and the multi-step loss in the fused ANIL call (mi_meta_batch_anil_lr, mi_meta_batch_anil_steps,
include/mi_maml.h) on the GPU: against the fp64 oracle whose objective is sum_j w_j CE(query at theta_j) with step-size
leaves (tests/anil_steps_oracle.py), the bitwise relations to the plain call, the launch make-up, graph replay with the operands
overwritten in place, the BatchNorm export and the Python surface.  Shapes (anil_steps_oracle.SHAPES): the Omniglot ANIL trunk 5-way
1-shot (Ph = 645) at T = 1 and T = 3, 3-way 2-shot (Ph = 387), and the Mini-ImageNet ANIL trunk 5-way 5-shot (Ph = 8005, the 5x5 column
permutation of the head weight) at T = 2."""
import functools

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.engine import MetaEngine, ModelSpec
from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from gpu_utils import rel_err, report
import anil_steps_oracle as A

pytestmark = pytest.mark.gpu

BASE_LR = 0.4


def _mspec(shape):
    _, (hidden, channels, max_pool), hw, _, ways, _ = A.SHAPES[shape]
    return ModelSpec.anil(ways, hidden=hidden, channels=channels, max_pool=max_pool, in_hw=hw)


def _inputs(shape, ids=None):
    """(engine spec, theta, data [T, 2n, C, H, W], labels, fc, ways, shots) on the GPU."""
    dataset, (_, channels, _), hw, fc, ways, shots = A.SHAPES[shape]
    _, tf, th, _, _, _ = A.fixtures(shape)
    theta = torch.cat([R.flatten_params(tf), R.flatten_params(th)]).float().cuda().contiguous()
    data, labels = synthetic.make_meta_batch(dataset, ids if ids is not None else A.GPU_TASKS[shape], ways, shots)
    data = torch.from_numpy(data).reshape(data.shape[0], data.shape[1], channels, hw, hw).cuda().contiguous()
    return _mspec(shape), theta, data, torch.from_numpy(labels).cuda().contiguous(), fc, ways, shots


def _np(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.detach().cpu().numpy().copy() for t in ts)


def _w(*ws):
    return torch.tensor(ws, dtype=torch.float32, device='cuda')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _steps(eng, theta, data, labels, shots, K, w, lr, **kw):
    """meta_batch_anil_steps with a scalar step (lr a number) or a vector (an array); numpy (loss, acc, grad, lr_grad, logits)."""
    step = dict(inner_lr=float(lr)) if np.ndim(lr) == 0 else dict(lr_vec=_dev(lr))
    return _np(*eng.meta_batch_anil_steps(theta, data, labels, shots, K, w, return_logits=True, **step, **kw))


def _same(tag, names, got, want):
    for name, a, b in zip(names, got, want):
        assert (a is None and b is None) or np.array_equal(a, b), (tag, name, rel_err(a, b))


# ---------------------------------------------------------------------------------------------------------------- 1
ORACLE_CASES = A.ORACLE_CASES
LOSS_FLOOR = 1e-4


_case_lr = A.case_lr


@functools.lru_cache(maxsize=None)
def _oracle(case, fp64):
    """One oracle run per case and precision, shared by every test that needs it (never modified)."""
    return A.case_oracle(case, torch.float64 if fp64 else torch.float32)


def _held(name, err, ref_err, floor):
    """The project's rule: err <= max(floor, 2 x the fp32 oracle's own error on the same inputs)."""
    print(f'[held] {name}: err {np.max(err):.3e} fp32-oracle err {np.max(ref_err):.3e} floor {floor:.0e}')
    assert np.all(np.asarray(err) <= np.maximum(floor, 2 * np.asarray(ref_err))), (name, err, ref_err, floor)


def _run_case(eng, case, **kw):
    shape, ids, K, entry, kind, fo, w, _ = ORACLE_CASES[case]
    _, theta, data, labels, _, _, shots = _inputs(shape, list(ids))
    lr = _case_lr(case)
    if entry == 'lr':
        return _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, _dev(lr), first_order=fo, want_lr_grad=True, return_logits=True, **kw))
    return _steps(eng, theta, data, labels, shots, K, _w(*w), lr, first_order=fo, want_lr_grad=kind != 'scalar', **kw)


def _check_vs_oracle(tag, case, got):
    loss, acc, grad, lr_grad, logits = got
    shape, ids, K, entry, kind, _, _, floor = ORACLE_CASES[case]
    o64, o32 = _oracle(case, True), _oracle(case, False)
    rows = slice(K, K + 1) if entry == 'lr' else slice(0, K + 1)
    if entry == 'lr':
        loss, acc, logits = loss[None], acc[None], logits[None]
    l64 = o64['losses'][rows]
    nf = o64['grad_feat'].size
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), trunk=rel_err(grad[:nf], o64['grad_feat']), head=rel_err(grad[nf:], o64['grad_head']))
    refs = dict(loss=np.abs(o32['losses'][rows] - l64) / np.abs(l64), trunk=rel_err(o32['grad_feat'], o64['grad_feat']),
                head=rel_err(o32['grad_head'], o64['grad_head']))
    if kind != 'scalar':
        assert lr_grad.shape == o64['lr_grad'].shape
        errs['lr_grad'], refs['lr_grad'] = rel_err(lr_grad, o64['lr_grad']), rel_err(o32['lr_grad'], o64['lr_grad'])
    report(f'anil_steps_oracle[{case}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           trunk_rel_err=errs['trunk'], head_rel_err=errs['head'], ref_fp32_trunk_rel_err=refs['trunk'], ref_fp32_head_rel_err=refs['head'],
           lr_grad_rel_err=errs.get('lr_grad', 0.0), ref_fp32_lr_grad_rel_err=refs.get('lr_grad', 0.0))
    _held('loss', errs['loss'], refs['loss'], LOSS_FLOOR)
    # trunk and head gradients: the existing bars of tests/test_gpu_anil.py for the same trunk, as they stand
    assert errs['trunk'] < floor and errs['head'] < floor, (errs['trunk'], errs['head'], floor)
    if kind != 'scalar':
        _held('lr_grad', errs['lr_grad'], refs['lr_grad'], floor)
    # per-step accuracy: equal on the rows whose fp64 top-2 margin is clear; at most one row in ten of a (step, task) may be unclear
    lo64 = o64['logits'][rows]
    clear = A.clear_rows(lo64)
    assert np.all((~clear).sum(axis=-1) * 10 <= clear.shape[-1]), (~clear).sum(axis=-1)
    assert np.array_equal(logits.argmax(axis=-1)[clear], lo64.argmax(axis=-1)[clear])
    full = clear.all(axis=-1)
    assert np.array_equal(acc[full], o64['accs'][rows][full].astype(np.float32))


@pytest.mark.parametrize('case', list(ORACLE_CASES))
def test_against_the_fp64_oracle(conv_form, case):
    """Every operand form: the per-step losses within max(1e-4, 2 x the fp32 oracle's error), the trunk and head gradients under the
    plain ANIL call's bars, lr_grad within max(that bar, 2 x the fp32 oracle's error), accuracy equal where the fp64 margin is clear."""
    _check_vs_oracle(conv_form, case, _run_case(MetaEngine(_mspec(ORACLE_CASES[case][0])), case))


# ---------------------------------------------------------------------------------------------------------------- 2
NAMES = ('loss', 'acc', 'grad', 'logits')


@pytest.mark.parametrize('shape,K', [('omni', 2), ('omni', 3), ('omni3w2s', 2), ('min', 2)])
def test_uniform_vector_is_the_plain_call(shape, K):
    """A uniform lr_vec: the plain call's loss, accuracy, logits and first-order gradient bit for bit at any step, and its second-order
    gradient at the power-of-two steps 0.5 and 0.25 (D lam is then an exact scaling of lam)."""
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    eng = MetaEngine(mspec)
    Ph = A.head_count(fc, ways)
    for lr, fo in ((0.4, True), (0.5, False), (0.25, False), (0.5, True)):
        want = _np(*eng.meta_batch_anil(theta, data, labels, shots, K, lr, first_order=fo, return_logits=True))
        for rows in (1, K):
            vec = torch.full((rows, Ph), lr, dtype=torch.float32, device='cuda')
            l, a, g, lg, lo = _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec, first_order=fo, want_lr_grad=True, return_logits=True))
            _same((lr, fo, rows), NAMES, (l, a, g, lo), want)
            assert lg.shape == (rows, Ph) and np.isfinite(lg).all() and np.abs(lg).sum() > 0
    # second order at a step that is no power of two: same loss bits, the gradient to rounding
    want = _np(*eng.meta_batch_anil(theta, data, labels, shots, K, 0.4, return_logits=True))
    l, a, g, _, lo = _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, torch.full((1, Ph), 0.4, device='cuda'), return_logits=True))
    _same('0.4', ('loss', 'acc', 'logits'), (l, a, lo), (want[0], want[1], want[3]))
    assert rel_err(g, want[2]) < 1e-5
    # evaluation only
    want = _np(*eng.meta_batch_anil(theta, data, labels, shots, K, 0.4, with_grad=False, return_logits=True))
    got = _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, torch.full((1, Ph), 0.4, device='cuda'), with_grad=False, return_logits=True))
    assert got[2] is None and got[3] is None
    _same('eval', ('loss', 'acc', 'logits'), (got[0], got[1], got[4]), (want[0], want[1], want[3]))


@pytest.mark.parametrize('shape,K,fo', [('omni', 1, False), ('omni', 3, False), ('omni', 3, True), ('omni3w2s', 2, False), ('min', 2, False)])
def test_final_only_weights_and_trajectory_are_the_plain_calls(shape, K, fo):
    """w = (0, .., 0, 1) with a scalar step: row K and meta_grad have the plain call's bits.  Row j of any steps call is the plain call
    with adapt_steps = j and the same with_grad, j = 0..K."""
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    eng = MetaEngine(mspec)
    lr = 0.4
    want = _np(*eng.meta_batch_anil(theta, data, labels, shots, K, lr, first_order=fo, return_logits=True))
    l, a, g, lg, lo = _steps(eng, theta, data, labels, shots, K, _w(*([0.0] * (K - 1) + [1.0])), lr, first_order=fo)
    assert l.shape == a.shape == (K + 1, data.shape[0]) and lo.shape == (K + 1, data.shape[0], ways * shots, ways) and lg is None
    _same('final_only', NAMES, (l[K], a[K], g, lo[K]), want)
    wts = _w(*np.linspace(0.2, 0.8, K))
    for with_grad in (True, False):
        l, a, g, _, lo = _steps(eng, theta, data, labels, shots, K, wts, lr, first_order=fo, with_grad=with_grad)
        assert (g is not None) == with_grad
        for j in range(K + 1):
            pj = _np(*eng.meta_batch_anil(theta, data, labels, shots, j, lr, first_order=fo, with_grad=with_grad, return_logits=True))
            _same(('row', j, with_grad), ('loss', 'acc', 'logits'), (l[j], a[j], lo[j]), (pj[0], pj[1], pj[3]))
    assert not np.array_equal(l[0], l[K])


def test_zero_steps_tasks_apart_and_repeatability():
    """An all-zero lr_vec leaves theta where it was: every loss row equals row 0.  A task's outputs do not depend on the other tasks of
    the call (T = 1 against T = 3; lr_grad and meta_grad are sums over the tasks).  Two identical calls agree in every output."""
    shape, K = 'omni', 3
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    eng = MetaEngine(mspec)
    Ph = A.head_count(fc, ways)
    w = _w(0.2, 0.3, 0.5)
    l, a, g, lg, lo = _steps(eng, theta, data, labels, shots, K, w, np.zeros((K, Ph), np.float32), want_lr_grad=True)
    for j in range(1, K + 1):
        _same(('zero', j), ('loss', 'acc', 'logits'), (l[j], a[j], lo[j]), (l[0], a[0], lo[0]))
    assert np.isfinite(lg).all() and np.abs(lg).sum() > 0            # a step of 0 still has a gradient
    vec = A.lr_vector(fc, ways, BASE_LR, K, 5, frozen=('bias',))
    whole = _steps(eng, theta, data, labels, shots, K, w, vec, want_lr_grad=True)
    again = _steps(eng, theta, data, labels, shots, K, w, vec, want_lr_grad=True)
    _same('repeat', ('loss', 'acc', 'grad', 'lr_grad', 'logits'), again, whole)
    singles = [_steps(eng, theta, data[t:t + 1].contiguous(), labels[t:t + 1].contiguous(), shots, K, w, vec, want_lr_grad=True)
               for t in range(data.shape[0])]
    for t, s in enumerate(singles):
        _same(('single', t), ('loss', 'acc', 'logits'), (s[0][:, 0], s[1][:, 0], s[4][:, 0]), (whole[0][:, t], whole[1][:, t], whole[4][:, t]))
    # the sums over tasks: the head's entries are plain fp32 sums in task order, the trunk's to rounding; lr_grad is one fp64 chain
    assert rel_err(np.sum([s[2].astype(np.float64) for s in singles], axis=0), whole[2]) < 1e-6
    assert rel_err(np.sum([s[3].astype(np.float64) for s in singles], axis=0), whole[3]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------- 3
def _census(eng, fn):
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    c = {f'{op}/{layer}': int(n) for (op, layer), (_, n) in eng.profile_collect().items()}
    eng.profile(False)
    return c


# the plain call's own census (Omniglot ANIL trunk, K = 2, second order, with the gradient): the launches of the head loop
PLAIN_HEAD_CENSUS = {'head_fwd_bwd/0': 3, 'head_tangent/0': 2, 'misc/2': 6, 'misc/3': 1}


def test_launch_make_up():
    """Against the plain call (K head steps): _lr adds 1 (step sizes into engine layout, misc/1) and 1 with lr_grad (fold, misc/3); its
    second-order recursion is one launch per step + 1 where the plain call makes two (misc/2: 1 - K), its first-order one makes none.
    _steps adds K head launches (the query set at theta_0..theta_{K-1}) and, with a gradient, K query-cotangent accumulations (misc/2),
    second order + 1 (lam_K = w_K q_K), first order + K (lam_k += w_k q_k and lam_K).  Identical at T = 1 and T = 3."""
    shape, K = 'omni', 2
    diffs = []
    for ids in ([0], [0, 1, 2]):
        mspec, theta, data, labels, fc, ways, shots = _inputs(shape, ids)
        eng = MetaEngine(mspec)
        vec = _dev(A.lr_vector(fc, ways, BASE_LR, K, 5))
        w = _w(0.3, 0.7)
        for fo in (False, True):
            base = _census(eng, lambda: eng.meta_batch_anil(theta, data, labels, shots, K, BASE_LR, first_order=fo))
            print(f'[census] plain ANIL call, T = {len(ids)}, first order {fo}: {sorted(base.items())}')
            if not fo:
                assert {k: base.get(k, 0) for k in PLAIN_HEAD_CENSUS} == PLAIN_HEAD_CENSUS, base
            calls = {
                'lr': (lambda: eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec, first_order=fo), {'misc/1': 1, 'misc/2': 0 if fo else 1 - K}),
                'lr+grad': (lambda: eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec, first_order=fo, want_lr_grad=True),
                            {'misc/1': 1, 'misc/3': 1, 'misc/2': 0 if fo else 1 - K}),
                'steps': (lambda: eng.meta_batch_anil_steps(theta, data, labels, shots, K, w, inner_lr=BASE_LR, first_order=fo),
                          {'head_fwd_bwd/0': K, 'misc/2': 2 * K if fo else 1}),
                'steps+vec+grad': (lambda: eng.meta_batch_anil_steps(theta, data, labels, shots, K, w, lr_vec=vec, first_order=fo, want_lr_grad=True),
                                   {'head_fwd_bwd/0': K, 'misc/1': 1, 'misc/3': 1, 'misc/2': 2 * K if fo else 1}),
            }
            for name, (fn, extra) in calls.items():
                got = _census(eng, fn)
                diff = {k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)}
                assert diff == {k: v for k, v in extra.items() if v}, (ids, fo, name, diff)
                diffs.append(diff)
        base = _census(eng, lambda: eng.meta_batch_anil(theta, data, labels, shots, K, BASE_LR, with_grad=False))
        got = _census(eng, lambda: eng.meta_batch_anil_steps(theta, data, labels, shots, K, w, inner_lr=BASE_LR, with_grad=False))
        diffs.append({k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)})
        assert diffs[-1] == {'head_fwd_bwd/0': K}
    assert diffs[:len(diffs) // 2] == diffs[len(diffs) // 2:]


# ---------------------------------------------------------------------------------------------------------------- 4
def test_graph_replay_reads_weights_and_step_sizes_from_the_device():
    """Eager, capture and a replay on the same buffers give identical bits; after step_w and lr_vec are overwritten IN PLACE the next
    (replayed) call equals a fresh eager engine on the new values."""
    shape, K = 'omni', 2
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    w, vec = _w(0.3, 0.7), _dev(A.lr_vector(fc, ways, BASE_LR, K, 5))
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    call = lambda e, ww, vv: _np(*e.meta_batch_anil_steps(theta, data, labels, shots, K, ww, lr_vec=vv, want_lr_grad=True, return_logits=True))
    first = call(eng, w, vec)
    for i in range(2):
        _same(('replay', i), ('loss', 'acc', 'grad', 'lr_grad', 'logits'), call(eng, w, vec), first)
    w.copy_(_w(0.6, 0.4))
    vec.copy_(_dev(A.lr_vector(fc, ways, 0.3, K, 9, frozen=('bias',))))
    replayed = call(eng, w, vec)
    fresh = call(MetaEngine(mspec), _w(0.6, 0.4), _dev(A.lr_vector(fc, ways, 0.3, K, 9, frozen=('bias',))))
    _same('in_place', ('loss', 'acc', 'grad', 'lr_grad', 'logits'), replayed, fresh)
    assert not np.array_equal(replayed[2], first[2]) and not np.array_equal(replayed[0][K], first[0][K])
    eng.set_graph(False)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_bn_export_is_the_plain_calls():
    """One trunk pass, one exported slot, the plain call's bits."""
    shape, K = 'omni', 2
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    T = data.shape[0]
    eng = MetaEngine(mspec)
    buf = eng.set_bn_export(T, 1)
    eng.meta_batch_anil(theta, data, labels, shots, K, BASE_LR)
    want = _np(buf)[0]
    for fn in (lambda: eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(0.5, 0.5), inner_lr=BASE_LR),
               lambda: eng.meta_batch_anil_lr(theta, data, labels, shots, K, _dev(A.lr_vector(fc, ways, BASE_LR, K, 5)))):
        buf.zero_()
        fn()
        got = _np(buf)[0]
        assert got.shape == (1, T, 2, mspec.hidden * mspec.n_layers) and np.abs(want).sum() > 0 and np.array_equal(got, want)
    eng.set_bn_export(0)


# ---------------------------------------------------------------------------------------------------------------- 6
def _learner(shape, lr):
    """(features, MAML head, trunk module) with the fixtures' parameters; lr: a number, or a function head -> InnerLR."""
    _, (hidden, channels, max_pool), _, fc, ways, _ = A.SHAPES[shape]
    _, tf, th, _, _, _ = A.fixtures(shape)
    trunk = cf.ConvBase(output_size=64, hidden=hidden, channels=channels, max_pool=max_pool)
    head = torch.nn.Linear(fc, ways)
    with torch.no_grad():
        for k, p in trunk.named_parameters():
            p.copy_(tf['0.' + k].float())
        head.weight.copy_(th['weight'].float())
        head.bias.copy_(th['bias'].float())
    features = torch.nn.Sequential(trunk).cuda()
    head = head.cuda()
    return features, cf.MAML(head, lr=lr(head) if callable(lr) else lr), head


def _grads(params):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params]).cpu().numpy()


def test_backward_fills_trunk_head_and_step_size_gradients():
    """meta_batch_adapt_anil through MAML(Linear, lr=InnerLR(per='tensor', steps=K, learnable=True)) -- which raised in float(inner_lr)
    before the vector call existed: .backward() leaves the engine call's meta_grad in the trunk's and the head's .grad and the per-tensor
    sums of its lr_grad in values.grad.  The same through meta_batch_adapt_anil_steps with weights; fast_adapt(..., features=) takes the
    vector call too."""
    shape, K = 'omni', 2
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    init = torch.tensor([[0.3, 0.5], [0.45, 0.2]])
    make = lambda head: cf.InnerLR(head, init, per='tensor', steps=K, learnable=True)
    features, maml, head = _learner(shape, make)
    il = maml.lr
    params = list(features.parameters()) + [head.weight, head.bias]
    eng = MetaEngine(mspec)
    flat = il.flat().detach().contiguous()

    def twin_grad(lg):          # the per-tensor sums, by the same expansion
        twin = make(head)
        (twin.flat() * torch.from_numpy(lg).cuda()).sum().backward()
        return twin.values.grad.cpu().numpy()

    total, losses, accs = cf.meta_batch_adapt_anil(maml.clone(), features, data, labels, K, shots, ways)
    assert not losses.requires_grad and tuple(losses.shape) == (data.shape[0],)
    total.backward()
    l, a, g, lg, _ = _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, flat, want_lr_grad=True))
    assert np.array_equal(_grads(params), g) and np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a)
    assert np.array_equal(il.values.grad.cpu().numpy(), twin_grad(lg)) and np.abs(lg).sum() > 0

    for p in params + [il.values]:
        p.grad = None
    w = (0.3, 0.7)
    objective, losses, accs = cf.meta_batch_adapt_anil_steps(maml.clone(), features, data, labels, K, shots, ways, step_weights=list(w))
    assert tuple(losses.shape) == tuple(accs.shape) == (K + 1, data.shape[0])
    objective.backward()
    l, a, g, lg, _ = _np(*eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(*w), lr_vec=flat, want_lr_grad=True))
    assert np.array_equal(_grads(params), g) and np.array_equal(_np(losses)[0], l) and np.array_equal(il.values.grad.cpu().numpy(), twin_grad(lg))
    want_obj = float((np.asarray(w, dtype=np.float32)[:, None] * l[1:]).sum())
    assert abs(objective.item() - want_obj) <= 1e-5 * abs(want_obj)
    with torch.no_grad():
        objective, losses2, _ = cf.meta_batch_adapt_anil_steps(maml.clone(), features, data, labels, K, shots, ways, step_weights=list(w))
    # (the evaluation-only call takes block 1's statistics by another fp32 route than the call with a backward half: each is held to the
    # loss floor 1e-4 against fp64, so the two agree within 2e-4)
    assert not objective.requires_grad and np.allclose(_np(losses2)[0], l, rtol=2e-4)

    for p in params + [il.values]:
        p.grad = None
    d, lab = data[0].cpu(), labels[0].cpu()
    loss, acc = cf.fast_adapt((d, lab), maml.clone(), torch.nn.CrossEntropyLoss(), K, shots, ways, torch.device('cuda'), features=features)
    loss.backward()
    l1, _, g1, lg1, _ = _np(*eng.meta_batch_anil_lr(theta, data[:1].contiguous(), labels[:1].contiguous(), shots, K, flat, want_lr_grad=True))
    assert loss.item() == l1[0] and np.array_equal(_grads(params), g1) and np.array_equal(il.values.grad.cpu().numpy(), twin_grad(lg1))


def test_steps_default_is_final_only_frozen_bias_and_evaluate_steps():
    """step_weights=None is (0, .., 0, 1): with a scalar-lr learner the gradient of meta_batch_adapt_anil bit for bit.  allow_nograd with a
    bias that does not require grad takes the vector call and leaves the bias where it was.  evaluate_steps(..., features=) returns the
    K + 1 trajectory means from one call."""
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    shape, K = 'omni', 2
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    features, maml, head = _learner(shape, 0.4)
    params = list(features.parameters()) + [head.weight, head.bias]
    objective, losses, _ = cf.meta_batch_adapt_anil_steps(maml.clone(), features, data, labels, K, shots, ways)
    objective.backward()
    got = _grads(params)
    for p in params:
        p.grad = None
    total, plain, _ = cf.meta_batch_adapt_anil(maml.clone(), features, data, labels, K, shots, ways)
    total.backward()
    assert np.array_equal(got, _grads(params)) and np.array_equal(_np(losses)[0][K], _np(plain)[0])
    # a frozen bias
    head.bias.requires_grad_(False)
    frozen = cf.MAML(head, lr=0.4, allow_nograd=True)
    _, fl, _ = cf.meta_batch_adapt_anil(frozen.clone(), features, data, labels, K, shots, ways)
    eng = MetaEngine(mspec)
    vec = np.full((1, A.head_count(fc, ways)), 0.4, np.float32)
    vec[:, ways * fc:] = 0.0
    want = _np(*eng.meta_batch_anil_lr(theta, data, labels, shots, K, _dev(vec)))
    assert np.array_equal(_np(fl)[0], want[0]) and not np.array_equal(_np(fl)[0], _np(plain)[0])
    head.bias.requires_grad_(True)
    # evaluate_steps with a trunk
    p = dict(meta_batch_size=3, adapt_steps=K, shots=shots, ways=ways)
    dataset = A.SHAPES[shape][0]

    class Tasks(SyntheticTasks):
        def sample(self):
            d, l = super().sample()
            return d.view(-1, 1, 28, 28), l
    per_step = cf.evaluate_steps(p, Tasks(dataset, ways, shots, 0), maml, torch.nn.CrossEntropyLoss(), torch.device('cuda'), features=features)
    assert isinstance(per_step, list) and len(per_step) == K + 1
    la = _np(*eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(0.0, 1.0), inner_lr=0.4, with_grad=False))
    assert per_step == pytest.approx([float(x) for x in la[1].astype(np.float64).mean(axis=1)], abs=1e-6)
    want_final = cf.evaluate(p, Tasks(dataset, ways, shots, 0), maml, torch.nn.CrossEntropyLoss(), torch.device('cuda'), features=features)
    assert per_step[K] == pytest.approx(want_final, abs=1e-6)


def test_argument_errors_come_before_any_launch():
    shape, K = 'omni', 2
    mspec, theta, data, labels, fc, ways, shots = _inputs(shape)
    Ph, T = A.head_count(fc, ways), data.shape[0]
    eng = MetaEngine(mspec)
    vec = _dev(A.lr_vector(fc, ways, BASE_LR, K, 5))
    eng.profile(True)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # wrong weight count
        eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(0.2, 0.3, 0.5), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # on the host
        eng.meta_batch_anil_steps(theta, data, labels, shots, K, torch.tensor([0.3, 0.7]), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # wrong dtype
        eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(0.3, 0.7).double(), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='adapt_steps >= 1'):
        eng.meta_batch_anil_steps(theta, data, labels, shots, 0, _w(1.0), inner_lr=0.4)
    with pytest.raises(ValueError, match='exactly one of'):
        eng.meta_batch_anil_steps(theta, data, labels, shots, K, _w(0.3, 0.7))
    with pytest.raises(_lib.MiError, match='lr_vec must be'):                     # the whole model's count, not the head's
        eng.meta_batch_anil_lr(theta, data, labels, shots, K, torch.full((1, eng.param_count), 0.4, device='cuda'))
    with pytest.raises(_lib.MiError, match='lr_vec must be'):                     # three rows for two steps
        eng.meta_batch_anil_lr(theta, data, labels, shots, K, torch.full((3, Ph), 0.4, device='cuda'))
    with pytest.raises(_lib.MiError, match='lr_vec must be'):
        eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec.cpu())
    with pytest.raises(_lib.MiError, match='lr_vec must be'):
        eng.meta_batch_anil_lr(theta, data, labels, shots, K, vec.double())
    # the library's own checks, reached without the wrapper's: outputs stay as they were
    P = eng.param_count
    import ctypes as C
    nbytes = C.c_size_t()
    assert eng.lib.mi_anil_workspace_bytes_steps(eng._h, T, ways, shots, K, 1, 1, K, 1, 1, C.byref(nbytes)) == 0
    assert eng.lib.mi_anil_workspace_bytes_steps(eng._h, T, ways, shots, K, 1, 1, 3, 1, 1, C.byref(nbytes)) == -1      # lr_steps 3 for K = 2
    ws = eng._workspace(nbytes.value)
    out = torch.full((P + 6 * T + K * Ph,), -7.0, device='cuda')
    w = _w(0.3, 0.7)
    lo, ac, lrg = out[P:].data_ptr(), out[P + 3 * T:].data_ptr(), out[P + 6 * T:].data_ptr()
    lr_args = lambda k, vp, ls, wg, lg: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), T, ways, shots, k, vp, ls, 1, wg,
                                         lo, ac, out.data_ptr(), lg, None, ws.data_ptr(), ws.numel())
    st_args = lambda k, vp, ls, wp, wg, lg: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), T, ways, shots, k, 0.4, vp, ls, wp,
                                             1, wg, lo, ac, out.data_ptr(), lg, None, ws.data_ptr(), ws.numel())
    v = vec.data_ptr()
    for fn, a, text in (
            (eng.lib.mi_meta_batch_anil_lr, lr_args(K, None, 1, 1, None), 'lr_vec is NULL: mi_meta_batch_anil_lr'),
            (eng.lib.mi_meta_batch_anil_lr, lr_args(K, v, 3, 1, None), 'mi_meta_batch_anil_lr: lr_steps = 3 must be 1 or adapt_steps = 2'),
            (eng.lib.mi_meta_batch_anil_lr, lr_args(0, v, 2, 1, None), 'lr_steps = 2 must be 1 or adapt_steps = 0 (without inner steps: 1)'),
            (eng.lib.mi_meta_batch_anil_lr, lr_args(K, v, K, 0, lrg), 'mi_meta_batch_anil_lr: lr_grad_out given but with_grad = 0'),
            (eng.lib.mi_meta_batch_anil_steps, st_args(K, None, 0, None, 1, None), 'step_w is NULL: mi_meta_batch_anil_steps'),
            (eng.lib.mi_meta_batch_anil_steps, st_args(0, None, 0, w.data_ptr(), 1, None), 'mi_meta_batch_anil_steps needs adapt_steps >= 1, got 0'),
            (eng.lib.mi_meta_batch_anil_steps, st_args(K, None, 0, w.data_ptr(), 1, lrg), 'mi_meta_batch_anil_steps: lr_grad_out given without lr_vec'),
            (eng.lib.mi_meta_batch_anil_steps, st_args(K, v, 3, w.data_ptr(), 1, None), 'mi_meta_batch_anil_steps: lr_steps = 3 must be 1 or adapt_steps = 2'),
            (eng.lib.mi_meta_batch_anil_steps, st_args(K, v, K, w.data_ptr(), 0, lrg), 'mi_meta_batch_anil_steps: lr_grad_out given but with_grad = 0')):
        assert fn(*a) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode(), eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(T, K)
    assert eng.lib.mi_meta_batch_anil_lr(*lr_args(K, v, K, 1, None)) == -1
    assert 'the debug trace does not cover mi_meta_batch_anil_lr' in eng.lib.mi_last_error(eng._h).decode()
    assert eng.lib.mi_meta_batch_anil_steps(*st_args(K, None, 0, w.data_ptr(), 1, None)) == -1
    assert 'the debug trace does not cover mi_meta_batch_anil_steps' in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(0)
    pooled = MetaEngine(ModelSpec.omniglot(ways))                       # a mean-pooled head is not an ANIL head
    with pytest.raises(_lib.MiError, match='mean-pooled'):
        pooled.meta_batch_anil_lr(torch.zeros(pooled.param_count, device='cuda'), data, labels, shots, K, torch.full((1, 64 * ways + ways), 0.4, device='cuda'))
    torch.cuda.synchronize()
    assert eng.profile_collect() == {} and bool((out == -7.0).all())
    eng.profile(False)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_driver_runs_with_learnable_steps_and_the_multi_step_loss(tmp_path):
    """vision.anil_vision main on the Omniglot shape for two iterations: the first on the multi-step-loss call with annealed weights, the
    second on the plain vector call; the learnable step sizes move, finite losses, inner_lr.pt beside head.pt."""
    import math
    import os
    from exploring_meta_amd.vision import anil_vision
    logs = []
    (features, head), metrics = anil_vision.main(['--dataset', 'omni', '--shots', '1', '--adapt_steps', '2', '--meta_batch_size', '3',
                                                  '--num_iterations', '2', '--inner_lr', '0.4', '--inner_lr_per', 'tensor', '--learn_inner_lr',
                                                  '--multi_step_loss', '--msl_iterations', '1', '--save_dir', str(tmp_path)], log=logs.append)
    assert len(logs) == 2 and all(math.isfinite(v) for v in metrics.values())
    assert isinstance(head.lr, cf.InnerLR) and head.lr.learnable and any(q is head.lr.values for q in head.parameters())
    values = head.lr.values.detach().cpu()
    assert torch.isfinite(values).all() and not torch.all(values == 0.4)
    assert os.path.exists(tmp_path / 'head.pt') and os.path.exists(tmp_path / 'inner_lr.pt')
    assert torch.equal(torch.load(tmp_path / 'inner_lr.pt')['values'].cpu(), values)
