"""Multi-step loss and per-step query metrics in the fused MAML call (mi_meta_batch_maml_steps, include/mi_maml.h)
on the GPU: against the existing calls (final-only weights, the per-step trajectory), the fp64 oracle whose objective is
sum_j w_j CE(query at theta_j) (tests/msl_oracle.py) on every operand form and route, graph replay with the weights overwritten in place,
the BatchNorm export and the Python surface.  Shapes: Mini-ImageNet net 5-way 1-shot tasks 0..2, Omniglot net 5-way 1-shot tasks 0, 1."""
import functools

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
import msl_oracle as M

pytestmark = pytest.mark.gpu

WAYS, SHOTS = 5, 1
TASKS = {'min': [0, 1, 2], 'omni': [0, 1]}


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
    return M.lr_vector(_specs(net)[0], base, K, 5)


def _steps_call(eng, theta, data, labels, K, w, lr, **kw):
    """meta_batch_steps with a scalar step (lr a number) or a vector (lr an array); numpy (loss, acc, grad, lr_grad, logits)."""
    if np.ndim(lr) == 0:
        return _np(*eng.meta_batch_steps(theta, data, labels, SHOTS, K, w, inner_lr=float(lr), return_logits=True, **kw))
    return _np(*eng.meta_batch_steps(theta, data, labels, SHOTS, K, w, lr_vec=torch.from_numpy(lr).cuda(), return_logits=True, **kw))


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
def test_final_only_weights_are_the_existing_call(net, K, fo, lr, grad_tasks, switch, graph):
    """w = (0, .., 0, 1): the last step's loss, accuracy and logits, the meta-gradient and (vector form) lr_grad have the bits of
    meta_batch / meta_batch_lr with the same arguments -- the weighted terms enter as fmaf(w, q, x) behind the unchanged update, and
    1 * q = q.  With graph replay: the eager call, the capture and a replay."""
    _, mspec, theta, data, labels = _inputs(net)
    w = _w(*([0.0] * (K - 1) + [1.0]))
    vec = _vec(net, K, lr)
    engines = []
    for _ in range(2):                                   # one engine per call kind: a graph-mode engine hands out persistent outputs
        eng = MetaEngine(mspec)
        if switch:
            getattr(eng, switch[0])(switch[1])
        eng.set_graph(graph)
        engines.append(eng)
    plain, steps = engines
    for rep in range(3 if graph else 1):
        want = _np(*plain.meta_batch(theta, data, labels, SHOTS, K, lr, first_order=fo, return_logits=True, grad_tasks=grad_tasks))
        loss, acc, grad, _, logits = _steps_call(steps, theta, data, labels, K, w, lr, first_order=fo, grad_tasks=grad_tasks)
        assert loss.shape == acc.shape == (K + 1, data.shape[0]) and logits.shape == (K + 1, data.shape[0], WAYS * SHOTS, WAYS)
        for name, a, b in zip(('loss', 'acc', 'grad', 'logits'), (loss[K], acc[K], grad, logits[K]), want):
            assert np.array_equal(a, b), ('scalar', rep, name, rel_err(a, b))
        vt = torch.from_numpy(vec).cuda()
        want = _np(*plain.meta_batch_lr(theta, data, labels, SHOTS, K, vt, first_order=fo, grad_tasks=grad_tasks, want_lr_grad=True,
                                        return_logits=True))
        loss, acc, grad, lr_grad, logits = _steps_call(steps, theta, data, labels, K, w, vec, first_order=fo, grad_tasks=grad_tasks,
                                                       want_lr_grad=True)
        for name, a, b in zip(('loss', 'acc', 'grad', 'lr_grad', 'logits'), (loss[K], acc[K], grad, lr_grad, logits[K]), want):
            assert np.array_equal(a, b), ('vector', rep, name, rel_err(a, b))
        assert np.isfinite(lr_grad).all() and np.abs(lr_grad).sum() > 0 and np.abs(grad).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('net,fused1', [('min', 2), ('min', 0), ('omni', 2), ('min', 1), ('omni', 1)])
def test_trajectory_is_the_plain_calls(net, fused1):
    """grad_tasks = 0, K = 3 at step 0.1: loss, accuracy and logits after j steps are those of the plain evaluation call with
    adapt_steps = j, bit for bit, j = 0..3 -- one call in place of four, K support passes in place of K (K + 1) / 2.

    Bit for bit wherever the plain calls agree among themselves, which is a property of the EXISTING calls: a plain call takes block 1's
    statistics from the input Gram matrix only when it sweeps the support set at least twice (make_plan: adapt_steps >= 2 in an evaluation
    call), so with the Gram route on (set_fused_block1(1), the default) the plain calls with adapt_steps = 0, 1 round block 1 otherwise than
    those with adapt_steps = 2, 3 -- already theta_1 differs between the plain calls 1 and 3, and no single K = 3 run can have the bits of
    both.  (Measured on the MI355X, Mini-ImageNet net: loss 1.7e-7, logits 8.4e-7 relative at j = 0.)  So: on the routes without the Gram
    matrix (set_fused_block1(2) and (0)) every j is bit-equal; on the default route j = 2, 3 are bit-equal and j = 0, 1 -- two fp32 routes
    of the same mathematics, each held to the loss floor 1e-4 of test_gpu_engine.py's CASES against fp64 -- agree within 2e-4, with the
    accuracy equal."""
    K, lr = 3, 0.1
    _, mspec, theta, data, labels = _inputs(net)
    eng = MetaEngine(mspec)
    eng.set_fused_block1(fused1)
    loss, acc, grad, _, logits = _steps_call(eng, theta, data, labels, K, _w(0.2, 0.3, 0.5), lr, grad_tasks=0)
    assert grad is None
    for j in range(K + 1):
        want = _np(*eng.meta_batch(theta, data, labels, SHOTS, j, lr, with_grad=False, return_logits=True))
        print(f'[trajectory] {net} fused_block1={fused1} step {j}: loss rel {rel_err(loss[j], want[0]):.3e} logits rel '
              f'{rel_err(logits[j], want[3]):.3e} acc equal {np.array_equal(acc[j], want[1])}')
        for name, a, b in zip(('loss', 'acc', 'logits'), (loss[j], acc[j], logits[j]), (want[0], want[1], want[3])):
            if fused1 == 1 and j < 2 and name != 'acc':
                assert rel_err(a, b) <= 2e-4, (j, name, rel_err(a, b))
            else:
                assert np.array_equal(a, b), (j, name, rel_err(a, b))
    assert not np.array_equal(loss[0], loss[K])


def test_evaluate_steps_returns_the_trajectory_means():
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    net, K = 'min', 3
    model, _ = _model(net)
    maml = cf.MAML(model, lr=0.1)
    p = dict(meta_batch_size=3, adapt_steps=K, shots=SHOTS, ways=WAYS)
    got = cf.evaluate_steps(p, SyntheticTasks(net, WAYS, SHOTS, 0), maml, torch.nn.CrossEntropyLoss(), torch.device('cuda'))
    assert isinstance(got, list) and len(got) == K + 1
    want = []
    for j in range(K + 1):
        want.append(cf.evaluate(dict(p, adapt_steps=j), SyntheticTasks(net, WAYS, SHOTS, 0), maml, torch.nn.CrossEntropyLoss(), torch.device('cuda')))
    assert got == want


# ---------------------------------------------------------------------------------------------------------------- 3
ORACLE_CASES = {
    # name: net, K, step ('scalar' / 'vector'), base step, first order, weights, loss floor, gradient floor
    # (floors: the rows of test_gpu_engine.py's CASES with the same net and K; K = 3 at step 0.1 takes the K = 2, lr 0.1 row)
    'min_so_scalar': ('min', 2, 'scalar', 0.4, False, (0.3, 0.7), 1e-4, 2e-3),
    'min_so_vector': ('min', 2, 'vector', 0.4, False, (0.3, 0.7), 1e-4, 2e-3),
    'min_fo_vector': ('min', 2, 'vector', 0.4, True, (0.3, 0.7), 1e-4, 2e-3),
    'omni_so_scalar': ('omni', 2, 'scalar', 0.4, False, (0.3, 0.7), 1e-4, 1e-3),
    'min_K3_so_scalar': ('min', 3, 'scalar', 0.1, False, (0.2, 0.3, 0.5), 1e-4, 2e-3),
}


def _case_lr(case):
    net, K, kind, base = ORACLE_CASES[case][:4]
    return _vec(net, K, base) if kind == 'vector' else base


@functools.lru_cache(maxsize=None)
def _oracle(case, fp64, grad_tasks=None):
    """One oracle run per case, precision and train-task count, shared by every test and operand form that needs it (never modified)."""
    net, K, _, _, fo, w, _, _ = ORACLE_CASES[case]
    spec, _ = _specs(net)
    dtype = torch.float64 if fp64 else torch.float32
    datas, labels = task_tensors(net, TASKS[net], WAYS, SHOTS, dtype)
    return M.meta_batch(model_params(spec, 11), spec, datas, labels, K, SHOTS, WAYS, _case_lr(case), w, fo, dtype, grad_tasks)


def _held(name, err, ref_err, floor):
    """The rule of test_gpu_engine.py: err <= max(floor, 2 x the fp32 oracle's own error on the same inputs)."""
    assert np.all(np.asarray(err) <= np.maximum(floor, 2 * np.asarray(ref_err))), (name, err, ref_err, floor)


def _check_vs_oracle(tag, case, got, grad_tasks=None, check_acc=True):
    loss, acc, grad, lr_grad, logits = got
    _, K, kind, _, _, _, loss_floor, grad_floor = ORACLE_CASES[case]
    o64, o32 = _oracle(case, True, grad_tasks), _oracle(case, False, grad_tasks)
    errs = dict(loss=np.abs(loss - o64['losses']) / np.abs(o64['losses']), grad=rel_err(grad, o64['meta_grad']))
    refs = dict(loss=np.abs(o32['losses'] - o64['losses']) / np.abs(o64['losses']), grad=rel_err(o32['meta_grad'], o64['meta_grad']))
    if kind == 'vector':
        errs['lr_grad'], refs['lr_grad'] = rel_err(lr_grad, o64['lr_grad']), rel_err(o32['lr_grad'], o64['lr_grad'])
        assert lr_grad.shape == o64['lr_grad'].shape
    report(f'msl_oracle[{case}][{tag}]', loss_rel_err=float(errs['loss'].max()), ref_fp32_loss_rel_err=float(refs['loss'].max()),
           grad_rel_err=errs['grad'], ref_fp32_grad_rel_err=refs['grad'], lr_grad_rel_err=errs.get('lr_grad', 0.0),
           ref_fp32_lr_grad_rel_err=refs.get('lr_grad', 0.0))
    _held('loss', errs['loss'], refs['loss'], loss_floor)
    _held('grad', errs['grad'], refs['grad'], grad_floor)
    if kind == 'vector':
        _held('lr_grad', errs['lr_grad'], refs['lr_grad'], grad_floor)
    if not check_acc:
        return
    lo64 = o64['logits']
    for j in range(K + 1):
        for t in range(lo64.shape[1]):
            top2 = np.sort(lo64[j, t], axis=1)[:, -2:]
            clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * max(1.0, np.abs(lo64[j, t]).max())
            assert np.array_equal(logits[j, t].argmax(axis=1)[clear], lo64[j, t].argmax(axis=1)[clear]), (j, t)
            if clear.all():
                assert acc[j, t] == np.float32(o64['accs'][j, t]), (j, t)


def _run_case(eng, case, theta, data, labels, **kw):
    _, K, kind, _, fo, w, _, _ = ORACLE_CASES[case]
    return _steps_call(eng, theta, data, labels, K, _w(*w), _case_lr(case), first_order=fo, want_lr_grad=kind == 'vector', **kw)


@pytest.mark.parametrize('case', list(ORACLE_CASES))
def test_steps_call_vs_fp64_oracle(conv_form, case):
    """w = (0.3, 0.7) (K = 3: (0.2, 0.3, 0.5), two inner injections) on every operand form: the K + 1 per-step losses, the meta-gradient
    and lr_grad within max(floor, 2 x the fp32 oracle's own error), per-step accuracy equal where the fp64 top-2 margin is clear."""
    _, mspec, theta, data, labels = _inputs(ORACLE_CASES[case][0])
    _check_vs_oracle(conv_form, case, _run_case(MetaEngine(mspec), case, theta, data, labels))


# ---------------------------------------------------------------------------------------------------------------- 4
def test_routes_agree():
    """The case 'Mini-ImageNet, second order, vector' on the separate launches (set_fused_tail(0)), with and without graph replay, with
    grad_tasks = 2 of 3 and with the tasks one at a time: every run under the oracle bar; the routes whose fold order is the same (the
    one-launch advance and its separate launches, eager and replayed) give the same bits (as test_gpu_inner_lr_routes.py asserts for the
    vector call), and the per-step losses of all three tasks do not depend on how many of them are train tasks."""
    case = 'min_so_vector'
    _, mspec, theta, data, labels = _inputs('min')
    base = _run_case(MetaEngine(mspec), case, theta, data, labels)
    _check_vs_oracle('default', case, base)
    eng = MetaEngine(mspec)
    eng.set_fused_tail(0)
    unfused = _run_case(eng, case, theta, data, labels)
    _check_vs_oracle('fused_tail0', case, unfused)
    for name, a, b in zip(('loss', 'acc', 'grad', 'lr_grad', 'logits'), unfused, base):
        assert np.array_equal(a, b), ('fused_tail0', name, rel_err(a, b))
    for on in (0, 1):
        eng = MetaEngine(mspec)
        eng.set_graph(on)
        for rep in range(3 if on else 1):
            got = _run_case(eng, case, theta, data, labels)
            _check_vs_oracle(f'graph{on}', case, got)
            for name, a, b in zip(('loss', 'acc', 'grad', 'lr_grad', 'logits'), got, base):
                assert np.array_equal(a, b), (f'graph{on}', rep, name, rel_err(a, b))
    part = _run_case(MetaEngine(mspec), case, theta, data, labels, grad_tasks=2)
    _check_vs_oracle('grad_tasks2', case, part, grad_tasks=2)
    for name, a, b in zip(('loss', 'acc', 'logits'), (part[0], part[1], part[4]), (base[0], base[1], base[4])):
        assert np.array_equal(a, b), ('grad_tasks2', name)
    eng = MetaEngine(mspec)
    singles = [_run_case(eng, case, theta, data[t:t + 1].contiguous(), labels[t:t + 1].contiguous()) for t in range(data.shape[0])]
    summed = (np.concatenate([s[0] for s in singles], axis=1), np.concatenate([s[1] for s in singles], axis=1),
              np.sum([s[2].astype(np.float64) for s in singles], axis=0), np.sum([s[3].astype(np.float64) for s in singles], axis=0),
              np.concatenate([s[4] for s in singles], axis=1))
    _check_vs_oracle('one_at_a_time', case, summed)


# ---------------------------------------------------------------------------------------------------------------- 5
def test_graph_replay_reads_the_weights_from_the_device():
    """Eager, capture and a replay on the same buffers give identical bits; after step_w is overwritten IN PLACE the next (replayed)
    call equals a fresh eager engine on the new weights."""
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    w = _w(0.3, 0.7)
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    call = lambda e, ww: _np(*e.meta_batch_steps(theta, data, labels, SHOTS, K, ww, inner_lr=0.4, return_logits=True))
    first = call(eng, w)
    for i in range(2):
        for a, b in zip(call(eng, w), first):
            assert (a is None and b is None) or np.array_equal(a, b), i
    w.copy_(_w(0.6, 0.4))
    replayed = call(eng, w)
    fresh = MetaEngine(mspec)
    for name, a, b in zip(('loss', 'acc', 'grad', 'lr_grad', 'logits'), replayed, call(fresh, _w(0.6, 0.4))):
        assert (a is None and b is None) or np.array_equal(a, b), name
    assert not np.array_equal(replayed[2], first[2]) and np.array_equal(replayed[0], first[0])


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize('net,K', [('min', 2), ('omni', 3)])
def test_bn_export_is_the_plain_calls(net, K):
    """The intermediate query passes never write the BatchNorm export: the exported tensor has the adapt_steps + 1 passes of the plain call
    and its bits."""
    _, mspec, theta, data, labels = _inputs(net)
    T = data.shape[0]
    eng = MetaEngine(mspec)
    buf = eng.set_bn_export(T, K + 1)
    eng.meta_batch(theta, data, labels, SHOTS, K, 0.4)
    want = _np(buf)[0]
    buf.zero_()
    eng.meta_batch_steps(theta, data, labels, SHOTS, K, _w(*([1.0 / K] * K)), inner_lr=0.4)
    got = _np(buf)[0]
    eng.set_bn_export(0)
    assert got.shape == (K + 1, T, 2, mspec.hidden * mspec.n_layers) and np.abs(want).sum() > 0
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 7
def _model(net):
    theta = model_params(_specs(net)[0], 11)
    model = cf.OmniglotCNN(WAYS) if net == 'omni' else cf.MiniImagenetCNN(WAYS)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(theta[k].float())
    return model.cuda(), theta


def _grads(params):
    return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1) for p in params]).cpu().numpy()


def test_backward_fills_model_and_step_size_gradients():
    """objective.backward() through MAML(model, lr=InnerLR(per='tensor', steps=2, learnable=True)): the model's .grad is the engine call's
    meta_grad and the step sizes' .grad the per-tensor sums of its lr_grad; the objective is sum_t sum_j w_j loss[j, t]; the last row is
    what meta_batch_adapt returns.  Under no_grad the call only scores."""
    net, K, w = 'min', 2, (0.3, 0.7)
    _, _, theta, data, labels = _inputs(net)
    model, _ = _model(net)
    names = [n for n, _ in model.named_parameters()]
    init = torch.from_numpy(0.4 * (0.5 + synthetic.hash_uniform(21, (K, len(names))))).float()
    il = cf.InnerLR(model, init, per='tensor', steps=K, learnable=True, frozen=('base.0.',))
    maml = cf.MAML(model, lr=il)
    model.zero_grad()
    objective, losses, accs = cf.meta_batch_adapt_steps(maml.clone(), data, labels, K, SHOTS, WAYS, step_weights=list(w))
    assert tuple(losses.shape) == tuple(accs.shape) == (K + 1, data.shape[0]) and not losses.requires_grad
    objective.backward()
    grad, vgrad = _grads(model.parameters()), il.values.grad.cpu().numpy().copy()
    flat = il.flat().detach().contiguous()
    eng = model.engine()
    l, a, g, lg, _ = eng.meta_batch_steps(model.flat_parameters().detach().contiguous(), data, labels, SHOTS, K, _w(*w), lr_vec=flat,
                                          want_lr_grad=True)
    l, a, g, lg_np = _np(l, a, g, lg)
    assert np.array_equal(grad, g) and np.array_equal(_np(losses)[0], l) and np.array_equal(_np(accs)[0], a)
    twin = cf.InnerLR(model, init, per='tensor', steps=K, learnable=True, frozen=('base.0.',))      # the per-tensor sums, by the same expansion
    (twin.flat() * torch.from_numpy(lg_np).cuda()).sum().backward()
    assert np.array_equal(vgrad, twin.values.grad.cpu().numpy()) and np.abs(vgrad[:, 4:]).sum() > 0 and np.all(vgrad[:, :4] == 0)
    want_obj = float((np.asarray(w, dtype=np.float32)[:, None] * l[1:]).sum())
    assert abs(objective.item() - want_obj) <= 1e-5 * abs(want_obj)
    _, plain_losses, plain_accs = cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS)
    assert np.array_equal(_np(plain_losses)[0], l[K]) and np.array_equal(_np(plain_accs)[0], a[K])
    with torch.no_grad():
        objective, losses2, _ = cf.meta_batch_adapt_steps(maml.clone(), data, labels, K, SHOTS, WAYS, step_weights=list(w))
    assert not objective.requires_grad
    assert np.allclose(_np(losses2)[0], l, rtol=1e-6)         # evaluation-only forward: test_gpu_engine.py::test_eval_only_and_batching_equivalence
    with pytest.raises(RuntimeError):
        objective.backward()


def test_default_weights_are_final_only_and_scalar_learner():
    """step_weights=None is (0, .., 0, 1): the gradient of meta_batch_adapt, bit for bit, with a plain scalar-lr learner."""
    net, K = 'omni', 2
    _, _, _, data, labels = _inputs(net)
    model, _ = _model(net)
    maml = cf.MAML(model, lr=0.4)
    model.zero_grad()
    objective, losses, _ = cf.meta_batch_adapt_steps(maml.clone(), data, labels, K, SHOTS, WAYS)
    objective.backward()
    got = _grads(model.parameters())
    model.zero_grad()
    total, plain, _ = cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS)
    total.backward()
    assert np.array_equal(got, _grads(model.parameters())) and np.array_equal(_np(losses)[0][K], _np(plain)[0])
    assert objective.item() == pytest.approx(total.item(), rel=1e-6)


def test_argument_errors_come_before_any_launch():
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    eng = MetaEngine(mspec)
    eng.profile(True)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # wrong weight count
        eng.meta_batch_steps(theta, data, labels, SHOTS, K, _w(0.2, 0.3, 0.5), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='adapt_steps >= 1'):
        eng.meta_batch_steps(theta, data, labels, SHOTS, 0, _w(1.0), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # on the host
        eng.meta_batch_steps(theta, data, labels, SHOTS, K, torch.tensor([0.3, 0.7]), inner_lr=0.4)
    with pytest.raises(_lib.MiError, match='step_w must be'):                     # wrong dtype
        eng.meta_batch_steps(theta, data, labels, SHOTS, K, _w(0.3, 0.7).double(), inner_lr=0.4)
    with pytest.raises(ValueError, match='exactly one of'):
        eng.meta_batch_steps(theta, data, labels, SHOTS, K, _w(0.3, 0.7))
    # the library's own checks, reached without the wrapper's
    P = eng.param_count
    ws = eng._workspace(eng.workspace_bytes(3, SHOTS, K, True) + (64 << 20))
    out = torch.empty(P + 18, device='cuda')
    w = _w(0.3, 0.7)
    args = lambda k, wp, lrg: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), 3, 3, WAYS, SHOTS, k, 0.4, None, 0, wp, 1,
                               out[P:].data_ptr(), out[P + 9:].data_ptr(), out.data_ptr(), lrg, None, ws.data_ptr(), ws.numel())
    for a, text in ((args(0, w.data_ptr(), None), 'adapt_steps >= 1'), (args(K, None, None), 'step_w is NULL'),
                    (args(K, w.data_ptr(), out.data_ptr()), 'lr_grad_out given without lr_vec')):
        assert eng.lib.mi_meta_batch_maml_steps(*a) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(3, K)
    assert eng.lib.mi_meta_batch_maml_steps(*args(K, w.data_ptr(), None)) == -1
    assert 'debug trace' in eng.lib.mi_last_error(eng._h).decode()
    eng.set_trace(0)
    assert eng.profile_collect() == {}
    eng.profile(False)


def test_driver_runs_with_the_multi_step_loss():
    """vision.maml_vision main --multi_step_loss --msl_iterations 2 for 3 iterations on synthetic tasks: two iterations on the new call with
    annealed weights, the third on the plain call; finite losses, the logged ones being the last step's."""
    import math
    from exploring_meta_amd.vision import maml_vision
    logs = []
    model, metrics = maml_vision.main(['--dataset', 'omni', '--multi_step_loss', '--msl_iterations', '2', '--adapt_steps', '2',
                                       '--meta_batch_size', '4', '--num_iterations', '3', '--inner_lr', '0.4', '--inner_lr_per', 'tensor',
                                       '--learn_inner_lr', '--per_step_lr', '--freeze', 'base.0.'], log=logs.append)
    assert len(logs) == 3 and all(math.isfinite(v) for v in metrics.values()) and 0.0 <= metrics['test_acc'] <= 1.0
    assert all(torch.isfinite(q).all() for q in model.parameters())
