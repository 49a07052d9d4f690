"""Per-step parameter offsets in the fused MAML call (mi_meta_batch_maml_offsets, include/mi_maml.h) on the GPU:
all-zero offsets against the existing calls bit for bit, the fp64 oracle with the offsets as autograd leaves (tests/step_offsets_oracle.py)
on every operand form and route, graph replay with the offsets overwritten in place, the launch make-up, the Python surface
(``StepOffsets``, ``MAML(offsets=...)``), argument errors and the driver.  Shapes: Mini-ImageNet net 5-way 1-shot tasks 0..2, Omniglot net
5-way 1-shot tasks 0, 1."""
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
from helpers import model_params, task_tensors
from gpu_utils import rel_err, report
import step_offsets_oracle as S

pytestmark = pytest.mark.gpu

WAYS, SHOTS = 5, 1
TASKS = {'min': [0, 1, 2], 'omni': [0, 1]}
NAMES = ('loss', 'acc', 'grad', 'lr_grad', 'offsets_grad', 'logits')


def _specs(net):
    return (R.omniglot_spec(WAYS), ModelSpec.omniglot(WAYS)) if net == 'omni' else (R.mini_imagenet_spec(WAYS), ModelSpec.mini_imagenet(WAYS))


def _inputs(net, tasks=None):
    spec, mspec = _specs(net)
    theta = R.flatten_params(model_params(spec, 11)).float().cuda().contiguous()
    data, labels = synthetic.make_meta_batch(net, tasks or TASKS[net], WAYS, SHOTS)
    return spec, mspec, theta, torch.from_numpy(data).cuda().contiguous(), torch.from_numpy(labels).cuda().contiguous()


def _np(*ts):
    torch.cuda.synchronize()
    return tuple(None if t is None else t.detach().cpu().numpy().copy() for t in ts)


def _w(*ws):
    return torch.tensor(ws, dtype=torch.float32, device='cuda')


def _vec(net, K, base):
    """[K, P] step sizes: base * U(0.5, 1.5) per entry, block 1 frozen (tests/inner_lr_oracle.py)."""
    return S.lr_vector(_specs(net)[0], base, K, 5)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _call(eng, theta, data, labels, K, lr, ofs, w=None, **kw):
    """meta_batch_offsets with a scalar step (lr a number) or a vector (lr an array), ofs an array or a device tensor, w None or K weights;
    numpy (loss, acc, grad, lr_grad, offsets_grad, logits)."""
    ofs = ofs if torch.is_tensor(ofs) else _dev(ofs)
    w = None if w is None else (w if torch.is_tensor(w) else _w(*w))
    step = dict(inner_lr=float(lr)) if np.ndim(lr) == 0 else dict(lr_vec=_dev(lr))
    return _np(*eng.meta_batch_offsets(theta, data, labels, SHOTS, K, ofs, step_w=w, return_logits=True, **step, **kw))


def _same(tag, got, want, names):
    for name, a, b in zip(names, got, want):
        assert (a is None and b is None) or np.array_equal(a, b), (tag, name, None if a is None or b is None else rel_err(a, b))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('net,K,fo,lr,grad_tasks,switch,graph', [
    ('min', 2, False, 0.5, None, None, False),
    ('min', 2, True, 0.4, None, None, False),
    ('min', 2, False, 0.5, 2, None, False),
    ('min', 2, False, 0.5, None, ('set_fused_tail', 0), False),
    ('min', 2, False, 0.5, None, ('set_fused_block1', 0), False),
    ('omni', 1, False, 0.5, None, None, False),
    ('min', 2, False, 0.5, None, None, True),
    ('min', 2, True, 0.4, 2, None, True),
])
def test_zero_offsets_are_the_existing_calls(net, K, fo, lr, grad_tasks, switch, graph):
    """All-zero offsets: loss, accuracy, logits, the meta-gradient and lr_grad have the bits of meta_batch (scalar step, plain objective),
    meta_batch_lr (vector) and meta_batch_steps (multi-step loss, scalar and vector) with the same arguments -- the finished element is
    the unchanged update expression, and a zero offset selects it.  The rows of test_gpu_msl.py's final-only test: both orders, 2 train
    tasks of 3, the separate launches, block 1 without fusion, and graph replay (the eager call, the capture and a replay).  The offset
    gradient is asked for as well: it must not disturb the rest."""
    _, mspec, theta, data, labels = _inputs(net)
    T = data.shape[0]
    gt = T if grad_tasks is None else grad_tasks
    zero = torch.zeros(K, theta.numel(), device='cuda')
    vec = _vec(net, K, lr)
    vt = _dev(vec)
    w = _w(*([1.0] if K == 1 else [0.3, 0.7]))
    engines = []
    for _ in range(2):                                   # one engine per call kind: a graph-mode engine hands out persistent outputs
        eng = MetaEngine(mspec)
        if switch:
            getattr(eng, switch[0])(switch[1])
        eng.set_graph(graph)
        engines.append(eng)
    plain, offs = engines
    kw = dict(first_order=fo, grad_tasks=gt)
    for rep in range(3 if graph else 1):
        want = _np(*plain.meta_batch(theta, data, labels, SHOTS, K, lr, first_order=fo, return_logits=True, grad_tasks=gt))
        got = _call(offs, theta, data, labels, K, lr, zero, want_offsets_grad=True, **kw)
        assert got[0].shape == (T,) and got[5].shape == (T, WAYS * SHOTS, WAYS) and got[3] is None
        _same(('scalar', rep), (got[0], got[1], got[2], got[5]), want, ('loss', 'acc', 'grad', 'logits'))
        og_scalar = got[4]
        want = _np(*plain.meta_batch_lr(theta, data, labels, SHOTS, K, vt, want_lr_grad=True, return_logits=True, **kw))
        got = _call(offs, theta, data, labels, K, vec, zero, want_lr_grad=True, want_offsets_grad=True, **kw)
        _same(('vector', rep), (got[0], got[1], got[2], got[3], got[5]), want, ('loss', 'acc', 'grad', 'lr_grad', 'logits'))
        assert np.abs(got[3]).sum() > 0 and np.abs(got[2]).sum() > 0
        want = _np(*plain.meta_batch_steps(theta, data, labels, SHOTS, K, w, inner_lr=lr, return_logits=True, **kw))
        got = _call(offs, theta, data, labels, K, lr, zero, w=w, want_offsets_grad=True, **kw)
        assert got[0].shape == (K + 1, T) and got[5].shape == (K + 1, T, WAYS * SHOTS, WAYS)
        _same(('steps scalar', rep), (got[0], got[1], got[2], got[3], got[5]), want, ('loss', 'acc', 'grad', 'lr_grad', 'logits'))
        want = _np(*plain.meta_batch_steps(theta, data, labels, SHOTS, K, w, lr_vec=vt, want_lr_grad=True, return_logits=True, **kw))
        got = _call(offs, theta, data, labels, K, vec, zero, w=w, want_lr_grad=True, want_offsets_grad=True, **kw)
        _same(('steps vector', rep), (got[0], got[1], got[2], got[3], got[5]), want, ('loss', 'acc', 'grad', 'lr_grad', 'logits'))
        for og in (og_scalar, got[4]):
            assert og.shape == (K, theta.numel()) and np.isfinite(og).all() and np.abs(og).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 2
ORACLE_CASES = {
    # name: net, K, step ('scalar' / 'vector'), base step, first order, weights (None: the plain objective), offsets (std, tensors),
    #       loss floor, gradient floor (the floors of test_gpu_msl.py's ORACLE_CASES; the gradient floor also holds offsets_grad)
    'omni_K2_scalar': ('omni', 2, 'scalar', 0.4, False, (0.3, 0.7), (0.05, 'bn+bias'), 1e-4, 1e-3),
    'omni_K3_scalar': ('omni', 3, 'scalar', 0.4, False, (0.2, 0.3, 0.5), (0.05, 'bn+bias'), 1e-4, 1e-3),
    'min_K2_vector_so': ('min', 2, 'vector', 0.4, False, (0.3, 0.7), (0.05, 'bn+bias'), 1e-4, 2e-3),
    'min_K2_vector_fo': ('min', 2, 'vector', 0.4, True, (0.3, 0.7), (0.05, 'bn+bias'), 1e-4, 2e-3),
    'min_K2_vector_all': ('min', 2, 'vector', 0.4, False, (0.3, 0.7), (0.01, 'all'), 1e-4, 2e-3),
    'omni_K2_scalar_all': ('omni', 2, 'scalar', 0.4, False, (0.3, 0.7), (0.01, 'all'), 1e-4, 1e-3),
    'omni_K2_scalar_plain': ('omni', 2, 'scalar', 0.4, False, None, (0.05, 'bn+bias'), 1e-4, 1e-3),
}
ROUTE_CASE = 'min_K2_vector_so'


def _case_lr(case):
    net, K, kind, base = ORACLE_CASES[case][:4]
    return _vec(net, K, base) if kind == 'vector' else base


def _case_ofs(case, seed=31):
    net, K = ORACLE_CASES[case][:2]
    std, tensors = ORACLE_CASES[case][6]
    return S.offsets_array(_specs(net)[0], K, seed, std, tensors)


@functools.lru_cache(maxsize=None)
def _oracle(case, fp64, grad_tasks=None, seed=31):
    """One oracle run per case, precision, train-task count and offsets, shared by every test and operand form that needs it (never modified)."""
    net, K, _, _, fo, w = ORACLE_CASES[case][:6]
    spec, _ = _specs(net)
    dtype = torch.float64 if fp64 else torch.float32
    datas, labels = task_tensors(net, TASKS[net], WAYS, SHOTS, dtype)
    return S.meta_batch(model_params(spec, 11), spec, datas, labels, K, SHOTS, WAYS, _case_lr(case), w, _case_ofs(case, seed), fo, dtype, grad_tasks)


def _held(name, err, ref_err, floor):
    """The rule of test_gpu_engine.py: err <= max(floor, 2 x the fp32 oracle's own error on the same inputs)."""
    assert np.all(np.asarray(err) <= np.maximum(floor, 2 * np.asarray(ref_err))), (name, err, ref_err, floor)


def _check_vs_oracle(tag, case, got, grad_tasks=None, check_acc=True, seed=31):
    loss, acc, grad, lr_grad, ofs_grad, logits = got
    _, K, kind, _, _, w, _, loss_floor, grad_floor = ORACLE_CASES[case]
    o64, o32 = _oracle(case, True, grad_tasks, seed), _oracle(case, False, grad_tasks, seed)
    rows = slice(None) if w is not None else slice(K, K + 1)          # the plain objective: the call returns the last step only
    if w is None:
        loss, acc, logits = loss[None], acc[None], logits[None]
    l64, l32 = o64['losses'][rows], o32['losses'][rows]
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), grad=rel_err(grad, o64['meta_grad']), offsets_grad=rel_err(ofs_grad, o64['offsets_grad']))
    refs = dict(loss=np.abs(l32 - l64) / np.abs(l64), grad=rel_err(o32['meta_grad'], o64['meta_grad']),
                offsets_grad=rel_err(o32['offsets_grad'], o64['offsets_grad']))
    assert ofs_grad.shape == o64['offsets_grad'].shape
    if kind == 'vector':
        errs['lr_grad'], refs['lr_grad'] = rel_err(lr_grad, o64['lr_grad']), rel_err(o32['lr_grad'], o64['lr_grad'])
        assert lr_grad.shape == o64['lr_grad'].shape
    report(f'step_offsets_oracle[{case}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           grad_rel_err=errs['grad'], ref_fp32_grad_rel_err=refs['grad'], offsets_grad_rel_err=errs['offsets_grad'],
           ref_fp32_offsets_grad_rel_err=refs['offsets_grad'], lr_grad_rel_err=errs.get('lr_grad', 0.0),
           ref_fp32_lr_grad_rel_err=refs.get('lr_grad', 0.0))
    _held('loss', errs['loss'], refs['loss'], loss_floor)
    for name in ('grad', 'offsets_grad') + (('lr_grad',) if kind == 'vector' else ()):
        _held(name, errs[name], refs[name], grad_floor)
    if not check_acc:
        return
    lo64, a64 = o64['logits'][rows], o64['accs'][rows]
    for j in range(lo64.shape[0]):
        for t in range(lo64.shape[1]):
            top2 = np.sort(lo64[j, t], axis=1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * max(1.0, np.abs(lo64[j, t]).max())
            assert np.array_equal(logits[j, t].argmax(axis=1)[clear], lo64[j, t].argmax(axis=1)[clear]), (j, t)
            if clear.all():
                assert acc[j, t] == np.float32(a64[j, t]), (j, t)


def _run_case(eng, case, theta, data, labels, ofs=None, **kw):
    _, K, kind, _, fo, w = ORACLE_CASES[case][:6]
    return _call(eng, theta, data, labels, K, _case_lr(case), _case_ofs(case) if ofs is None else ofs, w=w, first_order=fo,
                 want_lr_grad=kind == 'vector', want_offsets_grad=True, **kw)


@pytest.mark.parametrize('case', list(ORACLE_CASES))
def test_offsets_call_vs_fp64_oracle(conv_form, case):
    """Offsets N(0, 0.05^2) on the BatchNorm tensors and linear.bias (two cases: N(0, 0.01^2) on every tensor, block 1's conv weights
    included, which pins the row workgroups' view of the shifted weights) on every operand form: the per-step losses, the meta-gradient,
    lr_grad and offsets_grad within max(floor, 2 x the fp32 oracle's own error), per-step accuracy equal where the fp64 top-2 margin is
    clear.  The offsets matter: the same call with zero offsets is far outside the bar."""
    net = ORACLE_CASES[case][0]
    _, mspec, theta, data, labels = _inputs(net)
    eng = MetaEngine(mspec)
    got = _run_case(eng, case, theta, data, labels)
    _check_vs_oracle(conv_form, case, got)
    if conv_form == 'split_bf16':
        without = _run_case(eng, case, theta, data, labels, ofs=np.zeros_like(_case_ofs(case)))
        moved = rel_err(without[2], got[2])
        print(f'[step_offsets] {case}: the offsets move the meta-gradient by {moved:.3f} relative')
        assert moved > 10 * ORACLE_CASES[case][8]               # ten times the gradient floor: a build that ignores the offsets fails the bar


# ---------------------------------------------------------------------------------------------------------------- 3
def test_routes_agree():
    """The Mini-ImageNet vector case on the separate launches (set_fused_tail(0)), with and without graph replay, with grad_tasks = 2 of 3
    and with the tasks one at a time: every run under the oracle bar; the one-launch advance and its separate launches, eager and
    replayed, give the same bits, offsets_grad included; one-at-a-time offsets_grad rows sum to the batched row within the fold's
    rounding -- each is one fp64 chain rounded once to fp32 (2^-24 relative per value), so the fp64 sum of three rounded values and the
    once-rounded sum differ by at most 4 * 2^-24 of the largest magnitude involved: 1e-6 relative in norm."""
    case = ROUTE_CASE
    _, mspec, theta, data, labels = _inputs('min')
    base = _run_case(MetaEngine(mspec), case, theta, data, labels)
    _check_vs_oracle('default', case, base)
    eng = MetaEngine(mspec)
    eng.set_fused_tail(0)
    unfused = _run_case(eng, case, theta, data, labels)
    _check_vs_oracle('fused_tail0', case, unfused)
    _same('fused_tail0', unfused, base, NAMES)
    for on in (0, 1):
        for tail in (1, 0):
            eng = MetaEngine(mspec)
            eng.set_fused_tail(tail)
            eng.set_graph(on)
            for rep in range(3 if on else 1):
                got = _run_case(eng, case, theta, data, labels)
                _check_vs_oracle(f'graph{on}_tail{tail}', case, got)
                _same((f'graph{on}_tail{tail}', rep), got, base, NAMES)
    part = _run_case(MetaEngine(mspec), case, theta, data, labels, grad_tasks=2)
    _check_vs_oracle('grad_tasks2', case, part, grad_tasks=2)
    _same('grad_tasks2', (part[0], part[1], part[5]), (base[0], base[1], base[5]), ('loss', 'acc', 'logits'))
    eng = MetaEngine(mspec)
    singles = [_run_case(eng, case, theta, data[t:t + 1].contiguous(), labels[t:t + 1].contiguous()) for t in range(data.shape[0])]
    f64sum = lambda i: np.sum([s[i].astype(np.float64) for s in singles], axis=0)
    summed = (np.concatenate([s[0] for s in singles], axis=1), np.concatenate([s[1] for s in singles], axis=1), f64sum(2), f64sum(3), f64sum(4),
              np.concatenate([s[5] for s in singles], axis=1))
    _check_vs_oracle('one_at_a_time', case, summed)
    e = rel_err(summed[4], base[4])
    print(f'[step_offsets] one-at-a-time offsets_grad against the batched fold: {e:.3e}')
    assert e <= 1e-6


def test_graph_replay_reads_the_offsets_from_the_device():
    """Eager, capture and a replay on the same buffers give identical bits; after offsets is overwritten IN PLACE the next (replayed) call
    equals a fresh eager engine on the new values."""
    case = ROUTE_CASE
    _, mspec, theta, data, labels = _inputs('min')
    ofs = _dev(_case_ofs(case))
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    first = _run_case(eng, case, theta, data, labels, ofs=ofs)
    for i in range(2):
        _same(('replay', i), _run_case(eng, case, theta, data, labels, ofs=ofs), first, NAMES)
    new = _case_ofs(case, seed=77)
    ofs.copy_(_dev(new))
    replayed = _run_case(eng, case, theta, data, labels, ofs=ofs)
    _same('in place', replayed, _run_case(MetaEngine(mspec), case, theta, data, labels, ofs=new), NAMES)
    assert not np.array_equal(replayed[2], first[2]) and not np.array_equal(replayed[0][1:], first[0][1:])
    assert np.array_equal(replayed[0][0], first[0][0])                               # theta_0 carries no offset


# ---------------------------------------------------------------------------------------------------------------- 4
def _census(eng, fn):
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    c = {f'{op}/{layer}': int(n) for (op, layer), (_, n) in eng.profile_collect().items()}
    eng.profile(False)
    return c


@pytest.mark.parametrize('fused_tail', [1, 0])
def test_launch_make_up(fused_tail):
    """Beyond the same call without offsets: + 1 (the offsets into engine layout: misc/1); with offsets_grad one fold per complete
    lam_{k+1} (misc/3: + K; a first-order call with the plain objective + 1, its lam is one constant); without the one-launch advance
    + K (the additions: misc/2).  The same at T = 1 and T = 3."""
    net, K = 'min', 2
    diffs = []
    for tasks in ([0], [0, 1, 2]):
        _, mspec, theta, data, labels = _inputs(net, tasks)
        eng = MetaEngine(mspec)
        eng.set_fused_tail(fused_tail)
        vec, w = _dev(_vec(net, K, 0.4)), _w(0.3, 0.7)
        ofs = _dev(S.offsets_array(_specs(net)[0], K, 31))
        for fo in (False, True):
            pairs = [
                (lambda: eng.meta_batch(theta, data, labels, SHOTS, K, 0.4, first_order=fo),
                 lambda og: eng.meta_batch_offsets(theta, data, labels, SHOTS, K, ofs, inner_lr=0.4, first_order=fo, want_offsets_grad=og), True),
                (lambda: eng.meta_batch_lr(theta, data, labels, SHOTS, K, vec, first_order=fo, want_lr_grad=True),
                 lambda og: eng.meta_batch_offsets(theta, data, labels, SHOTS, K, ofs, lr_vec=vec, first_order=fo, want_lr_grad=True,
                                                   want_offsets_grad=og), True),
                (lambda: eng.meta_batch_steps(theta, data, labels, SHOTS, K, w, lr_vec=vec, first_order=fo, want_lr_grad=True),
                 lambda og: eng.meta_batch_offsets(theta, data, labels, SHOTS, K, ofs, lr_vec=vec, step_w=w, first_order=fo, want_lr_grad=True,
                                                   want_offsets_grad=og), False),
            ]
            for without, with_offsets, plain_objective in pairs:
                base = _census(eng, without)
                for og in (False, True):
                    got = _census(eng, lambda: with_offsets(og))
                    diff = {k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)}
                    extra = {'misc/1': 1}
                    if og:
                        extra['misc/3'] = 1 if (fo and plain_objective) else K
                    if not fused_tail:
                        extra['misc/2'] = K
                    assert diff == extra, (tasks, fo, og, plain_objective, diff, extra)
                    diffs.append(diff)
    assert diffs[:len(diffs) // 2] == diffs[len(diffs) // 2:]


# ---------------------------------------------------------------------------------------------------------------- 5
def _model(net):
    theta = model_params(_specs(net)[0], 11)
    model = cf.OmniglotCNN(WAYS) if net == 'omni' else cf.MiniImagenetCNN(WAYS)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(theta[k].float())
    return model.cuda(), theta


def _grads(params):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params]).cpu().numpy()


def _bn_columns(model):
    cols, off = [], 0
    for n, p in model.named_parameters():
        if '.normalize.' in n:
            cols.extend(range(off, off + p.numel()))
        off += p.numel()
    return np.asarray(cols)


def _learner(net, K, seed=41):
    """MAML around the net with per-tensor learnable step sizes (BatchNorm frozen) and non-zero per-step BatchNorm offsets."""
    model, _ = _model(net)
    so = cf.StepOffsets(model, K)
    with torch.no_grad():
        so.values.copy_(torch.from_numpy((0.05 * np.random.RandomState(seed).standard_normal(tuple(so.values.shape))).astype(np.float32)))
    names = [n for n, _ in model.named_parameters()]
    init = torch.from_numpy(0.4 * (0.5 + synthetic.hash_uniform(21, (K, len(names))))).float()
    il = cf.InnerLR(model, init, per='tensor', steps=K, learnable=True, frozen=so.bn_prefixes())
    return model, il, so, cf.MAML(model, lr=il, offsets=so)


def test_backward_fills_model_step_size_and_offset_gradients():
    """objective.backward() through MAML(model, lr=InnerLR(per='tensor', steps=2, learnable=True, frozen=bn_prefixes),
    offsets=StepOffsets(model, 2)) with non-zero offsets: the model's .grad is the engine call's meta_grad, the step sizes' .grad the
    per-tensor sums of its lr_grad, the offsets' .grad the BatchNorm columns of its offsets_grad -- for the plain objective
    (meta_batch_adapt) and the multi-step loss (meta_batch_adapt_steps), also on the deferred-backward route.  Under no_grad the call
    scores only."""
    from exploring_meta_amd.core_functions import vision as V
    net, K, w = 'min', 2, (0.3, 0.7)
    _, _, _, data, labels = _inputs(net)
    model, il, so, maml = _learner(net, K)
    assert any(q is so.values for q in maml.parameters()) and any(q is il.values for q in maml.parameters())
    eng, cols = model.engine(), _bn_columns(model)
    theta = model.flat_parameters().detach().contiguous()
    flat, ofs = il.flat().detach().contiguous(), so.flat().detach().contiguous()
    assert float(flat[:, cols].abs().sum()) == 0.0 and float(ofs[:, cols].abs().min()) > 0.0

    def engine_call(step_w):
        return _np(*eng.meta_batch_offsets(theta, data, labels, SHOTS, K, ofs, lr_vec=flat, step_w=step_w, want_lr_grad=True,
                                           want_offsets_grad=True))

    def check(tag, adapt, step_w):
        for q in maml.parameters():
            q.grad = None
        objective, losses, accs = adapt()
        assert not losses.requires_grad
        objective.backward()
        grad, vgrad, ograd = _grads(model.parameters()), il.values.grad.cpu().numpy().copy(), so.values.grad.cpu().numpy().copy()
        l, a, g, lg, og, _ = engine_call(step_w)
        assert np.array_equal(grad, g), tag
        assert np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a), tag
        twin = cf.InnerLR(model, il.values.detach().clone(), per='tensor', steps=K, learnable=True, frozen=so.bn_prefixes())
        (twin.flat() * torch.from_numpy(lg).cuda()).sum().backward()                  # the per-tensor sums, by the same expansion
        assert np.array_equal(vgrad, twin.values.grad.cpu().numpy()) and np.abs(vgrad).sum() > 0, tag
        assert np.array_equal(ograd, og[:, cols]) and np.abs(ograd).sum() > 0, tag
        want = float(l.sum()) if step_w is None else float((np.asarray(w, dtype=np.float32)[:, None] * l[1:]).sum())
        assert abs(objective.item() - want) <= 1e-5 * abs(want), tag
        return l, a

    l_plain, a_plain = check('plain', lambda: cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS), None)
    l_steps, _ = check('steps', lambda: cf.meta_batch_adapt_steps(maml.clone(), data, labels, K, SHOTS, WAYS, step_weights=list(w)), _w(*w))
    assert np.array_equal(l_steps[K], l_plain)
    V.DEFERRED_OUTER_BACKWARD = True
    try:
        check('deferred', lambda: cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS), None)
    finally:
        V.DEFERRED_OUTER_BACKWARD = False
    with torch.no_grad():
        objective, losses2, _ = cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS)
    assert not objective.requires_grad
    assert np.allclose(_np(losses2)[0], l_plain, rtol=1e-6)       # evaluation-only forward: test_gpu_engine.py::test_eval_only_and_batching_equivalence
    with pytest.raises(RuntimeError):
        objective.backward()
    # the offsets reach the scores: the same learner without them scores otherwise
    _, plain_losses, _ = cf.meta_batch_adapt(cf.MAML(model, lr=il).clone(), data, labels, K, SHOTS, WAYS)
    assert not np.array_equal(_np(plain_losses)[0], l_plain)


def test_fast_adapt_and_evaluate_follow_the_offsets():
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    net, K = 'omni', 2
    model, il, so, maml = _learner(net, K)
    plain = cf.MAML(model, lr=il)
    loss, dev = torch.nn.CrossEntropyLoss(), torch.device('cuda')
    _, _, _, data, labels = _inputs(net)
    for q in maml.parameters():
        q.grad = None
    valid, acc = cf.fast_adapt((data[0].cpu(), labels[0].cpu()), maml.clone(), loss, K, SHOTS, WAYS, dev)
    valid.backward()
    l, a, g, _, og, _ = _np(*model.engine().meta_batch_offsets(model.flat_parameters().detach().contiguous(), data[:1].contiguous(),
                                                               labels[:1].contiguous(), SHOTS, K, so.flat().detach().contiguous(),
                                                               lr_vec=il.flat().detach().contiguous(), want_offsets_grad=True))
    assert valid.item() == pytest.approx(float(l[0]), rel=1e-6) and acc.item() == a[0]
    assert np.array_equal(_grads(model.parameters()), g) and np.array_equal(so.values.grad.cpu().numpy(), og[:, _bn_columns(model)])
    valid0, _ = cf.fast_adapt((data[0].cpu(), labels[0].cpu()), plain.clone(), loss, K, SHOTS, WAYS, dev)
    assert valid0.item() != valid.item()
    p = dict(meta_batch_size=3, adapt_steps=K, shots=SHOTS, ways=WAYS)
    got = cf.evaluate_steps(p, SyntheticTasks(net, WAYS, SHOTS, 0), maml, loss, dev)
    assert len(got) == K + 1 and got[K] == cf.evaluate(p, SyntheticTasks(net, WAYS, SHOTS, 0), maml, loss, dev)
    with torch.no_grad():
        _, losses, _ = cf.meta_batch_adapt_steps(maml.clone(), data, labels, K, SHOTS, WAYS)
        _, losses0, _ = cf.meta_batch_adapt_steps(plain.clone(), data, labels, K, SHOTS, WAYS)
    assert torch.equal(losses[0], losses0[0]) and not torch.equal(losses[1:], losses0[1:])     # theta_0 carries no offset


def test_wrong_row_count_anil_head_and_policies_are_refused():
    net = 'omni'
    model, _ = _model(net)
    _, _, _, data, labels = _inputs(net)
    maml = cf.MAML(model, lr=0.4, offsets=cf.StepOffsets(model, 3))
    eng = model.engine()
    eng.profile(True)
    with pytest.raises(ValueError, match='per-step offsets for 3 inner steps'):
        cf.meta_batch_adapt(maml.clone(), data, labels, 2, SHOTS, WAYS)
    with pytest.raises(ValueError, match='per-step offsets for 3 inner steps'):
        cf.meta_batch_adapt_steps(maml.clone(), data, labels, 2, SHOTS, WAYS)
    assert eng.profile_collect() == {}
    eng.profile(False)
    # an ANIL head
    head = torch.nn.Linear(64, WAYS).cuda()
    hm = cf.MAML(head, lr=0.4, offsets=cf.StepOffsets(head, 2, 'all'))
    with pytest.raises(NotImplementedError, match='per-step offsets are implemented for the fused MAML vision call'):
        cf.meta_batch_adapt_anil(hm.clone(), model.base, data.reshape(2, 10, 1, 28, 28), labels, 2, SHOTS, WAYS)
    with pytest.raises(NotImplementedError, match='per-step offsets are implemented for the fused MAML vision call'):
        cf.meta_batch_adapt_anil_steps(hm.clone(), model.base, data.reshape(2, 10, 1, 28, 28), labels, 2, SHOTS, WAYS)
    # a policy
    from exploring_meta_amd.core_functions import rl
    policy = cf.DiagNormalPolicy(2, 2).cuda()
    pm = cf.MAML(policy, lr=0.1, offsets=cf.StepOffsets(policy, 1, 'all'))
    with pytest.raises(NotImplementedError, match='per-step offsets are implemented for the fused MAML vision call'):
        rl._policy_lr_vector(pm.clone())
    with pytest.raises(NotImplementedError, match='per-step offsets are implemented for the fused MAML vision call'):
        pm.clone().adapt(torch.zeros((), device='cuda', requires_grad=True))


def test_stepwise_adapt_with_offsets_matches_the_fused_call():
    """learner.adapt x K with the same offsets (theta - lr * g + s_j, differentiated by autograd through mi_learner_hvp) gives the fused
    call's query loss, meta-gradient and offset gradient, and a further adapt is refused.  The bar is the one
    test_gpu_learner.py::test_stepwise_adapt_matches_oracle_and_fused holds its step-wise run to against the fused call after two steps:
    1e-2 relative."""
    net, K, lr, tol = 'omni', 2, 0.05, 1e-2
    model, _ = _model(net)
    so = cf.StepOffsets(model, K)
    with torch.no_grad():
        so.values.copy_(torch.from_numpy((0.05 * np.random.RandomState(43).standard_normal(tuple(so.values.shape))).astype(np.float32)))
    maml = cf.MAML(model, lr=lr, offsets=so)
    d, l = synthetic.make_task(net, 4, WAYS, SHOTS)
    ad, al, ed, el = cf.prepare_batch((torch.from_numpy(d), torch.from_numpy(l)), SHOTS, WAYS, torch.device('cuda'))
    loss = torch.nn.CrossEntropyLoss()
    learner = maml.clone()
    for _ in range(K):
        learner.adapt(loss(learner(ad), al))
    valid = loss(learner(ed), el)
    valid.backward()
    grad, ograd = _grads(model.parameters()), so.values.grad.cpu().numpy()
    fl, _, fg, _, fog, _ = _np(*model.engine().meta_batch_offsets(model.flat_parameters().detach().contiguous(),
                                                                  torch.from_numpy(d).cuda().unsqueeze(0).contiguous(),
                                                                  torch.from_numpy(l).cuda().unsqueeze(0).contiguous(), SHOTS, K,
                                                                  so.flat().detach().contiguous(), inner_lr=lr, want_offsets_grad=True))
    errs = dict(loss=abs(valid.item() - float(fl[0])) / abs(float(fl[0])), grad=rel_err(grad, fg), offsets_grad=rel_err(ograd, fog[:, _bn_columns(model)]))
    report('stepwise_offsets_vs_fused', **errs)
    assert all(e < tol for e in errs.values()), errs
    with pytest.raises(RuntimeError, match='offsets for 2 inner steps'):
        learner.adapt(loss(learner(ad), al))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_argument_errors_come_before_any_launch():
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    P = theta.numel()
    eng = MetaEngine(mspec)
    eng.profile(True)
    good = torch.zeros(K, P, device='cuda')
    for bad in (torch.zeros(K + 1, P, device='cuda'), torch.zeros(K, P - 1, device='cuda'), torch.zeros(K * P, device='cuda'),
                torch.zeros(K, P, device='cuda', dtype=torch.float64), torch.zeros(K, P), torch.zeros(P, K, device='cuda').t(),
                np.zeros((K, P), np.float32)):
        with pytest.raises(_lib.MiError, match='offsets must be'):
            eng.meta_batch_offsets(theta, data, labels, SHOTS, K, bad, inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='adapt_steps >= 1'):
        eng.meta_batch_offsets(theta, data, labels, SHOTS, 0, torch.zeros(0, P, device='cuda'), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='grad_tasks = 0'):
        eng.meta_batch_offsets(theta, data, labels, SHOTS, K, good, inner_lr=0.4, grad_tasks=0, want_offsets_grad=True)
    with pytest.raises(ValueError, match='exactly one of'):
        eng.meta_batch_offsets(theta, data, labels, SHOTS, K, good)
    with pytest.raises(ValueError, match='needs offsets'):
        eng.meta_batch_offsets(theta, data, labels, SHOTS, K, None, inner_lr=0.4)
    # the library's own checks, reached without the wrapper's
    ws = eng._workspace(eng.workspace_bytes(3, SHOTS, K, True) + (64 << 20))
    out = torch.empty(P + 18, device='cuda')
    og = torch.empty(K, P, device='cuda')
    args = lambda k, gt, op, lrg, ogp: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), 3, gt, WAYS, SHOTS, k, 0.4, None, 0,
                                        None, op, 1, out[P:].data_ptr(), out[P + 9:].data_ptr(), out.data_ptr(), lrg, ogp, None, ws.data_ptr(),
                                        ws.numel())
    for a, text in ((args(0, 3, good.data_ptr(), None, None), 'adapt_steps >= 1'), (args(K, 3, None, None, None), 'offsets is NULL'),
                    (args(K, 0, good.data_ptr(), None, og.data_ptr()), 'offsets_grad_out given but grad_tasks = 0'),
                    (args(K, 3, good.data_ptr(), out.data_ptr(), None), 'lr_grad_out given without lr_vec')):
        assert eng.lib.mi_meta_batch_maml_offsets(*a) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(3, K)
    assert eng.lib.mi_meta_batch_maml_offsets(*args(K, 3, good.data_ptr(), None, None)) == -1
    assert 'debug trace' in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(0)
    assert eng.profile_collect() == {}
    eng.profile(False)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_driver_runs_with_per_step_bn(tmp_path):
    """vision.maml_vision main --per_step_bn --multi_step_loss --msl_iterations 2 --first_order_iterations 1 --cosine_outer_lr for 3
    iterations on synthetic tasks: finite losses, the offsets have left zero, step_offsets.pt is written with --save_dir."""
    from exploring_meta_amd.vision import maml_vision
    logs = []
    model, metrics = maml_vision.main(['--dataset', 'omni', '--per_step_bn', '--multi_step_loss', '--msl_iterations', '2', '--adapt_steps', '2',
                                       '--first_order_iterations', '1', '--cosine_outer_lr', '--min_outer_lr', '1e-4', '--meta_batch_size', '4',
                                       '--num_iterations', '3', '--inner_lr', '0.4', '--save_dir', str(tmp_path)], log=logs.append)
    assert len(logs) == 3 and all(math.isfinite(v) for v in metrics.values()) and 0.0 <= metrics['test_acc'] <= 1.0
    assert all(torch.isfinite(q).all() for q in model.parameters())
    saved = torch.load(os.path.join(str(tmp_path), 'step_offsets.pt'))
    values = saved['values']
    assert tuple(values.shape) == (2, 8 * 64) and torch.isfinite(values).all()
    assert all(float(values[k].abs().sum()) > 0.0 for k in range(2))
    inner = torch.load(os.path.join(str(tmp_path), 'inner_lr.pt'))                   # the BatchNorm tensors left the inner loop: InnerLR(per='scalar')
    assert tuple(inner['values'].shape) == (1, 1)
