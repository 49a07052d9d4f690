"""Per-parameter, learnable inner-loop step sizes in the fused MAML call (mi_meta_batch_maml_lr, include/mi_maml.h) on the GPU:
against the scalar call (uniform vectors), the fp64 oracle with the update v - lr[name] * g (tests/inner_lr_oracle.py), the engine's own
debug trace, graph replay, the Python surface (InnerLR, MAML, allow_nograd, the step-wise learner), argument errors and launch make-up.
Shapes: Mini-ImageNet net 5-way 1-shot tasks 0..2 with K <= 2, Omniglot net 5-way 1-shot tasks 0, 1."""
import functools

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import vision as cf_vision
from exploring_meta_amd.engine import MetaEngine, ModelSpec
from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from helpers import model_params, task_tensors
from gpu_utils import rel_err, report
import inner_lr_oracle as O

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


def _steps(net, K, per_step):
    """The step sizes of the oracle cases: base * U(0.5, 1.5) per entry, block 1 frozen; base 0.5 for K = 1, 0.4 for K = 2."""
    return O.lr_vector(_specs(net)[0], 0.5 if K == 1 else 0.4, K if per_step else 1, 5)


@functools.lru_cache(maxsize=None)
def _oracle(net, K, per_step, fo, fp64):
    """One oracle run per case and precision, shared by every test and operand form that needs it (never modified)."""
    spec, _ = _specs(net)
    dtype = torch.float64 if fp64 else torch.float32
    datas, labels = task_tensors(net, TASKS[net], WAYS, SHOTS, dtype)
    return O.meta_batch(model_params(spec, 11), spec, datas, labels, K, SHOTS, WAYS, _steps(net, K, per_step), fo, dtype)


def _held(name, err, ref_err, floor):
    """The rule of test_gpu_engine.py: err <= max(floor, 2 x the fp32 oracle's own error on the same inputs)."""
    assert np.all(np.asarray(err) <= np.maximum(floor, 2 * np.asarray(ref_err))), (name, err, ref_err, floor)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize('net,K,fo,lr,grad_tasks,switch', [
    ('min', 2, False, 0.5, None, None),
    ('min', 2, True, 0.4, None, None),
    ('min', 2, False, 0.5, 2, None),
    ('min', 2, False, 0.5, None, ('set_fused_tail', 0)),
    ('min', 2, False, 0.5, None, ('set_fused_block1', 0)),
    ('omni', 1, False, 0.5, None, None),
])
def test_uniform_vector_is_the_scalar_call_bit_for_bit(net, K, fo, lr, grad_tasks, switch):
    """Loss, accuracy, meta-gradient and logits of a uniform vector, [1, P] and [K, P], equal the scalar call's bits.  theta_k, the
    losses and the first-order gradient do so for any step (same multiply and subtract per element).  The second-order recursion drives
    the Hessian-vector pass with D lam where the scalar call scales H lam afterwards: the same bits when the step is a power of two
    (every product and sum of the linear pass scales exactly), which is why the second-order cases run at 0.5."""
    _, mspec, theta, data, labels = _inputs(net)
    eng = MetaEngine(mspec)
    if switch:
        getattr(eng, switch[0])(switch[1])
    want = _np(*eng.meta_batch(theta, data, labels, SHOTS, K, lr, first_order=fo, return_logits=True, grad_tasks=grad_tasks))
    for steps in sorted({1, K}):
        vec = torch.full((steps, eng.param_count), lr, dtype=torch.float32, device='cuda')
        loss, acc, grad, lr_grad, logits = eng.meta_batch_lr(theta, data, labels, SHOTS, K, vec, first_order=fo, grad_tasks=grad_tasks,
                                                             want_lr_grad=True, return_logits=True)
        got = _np(loss, acc, grad, logits)
        for name, a, b in zip(('loss', 'acc', 'grad', 'logits'), got, want):
            assert np.array_equal(a, b), (name, steps, rel_err(a, b))
        lg = _np(lr_grad)[0]
        assert lg.shape == (steps, eng.param_count) and np.isfinite(lg).all() and np.abs(lg).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 2
ORACLE_CASES = [
    # net, K, per-step sizes, first order, loss floor, gradient floor (rows of test_gpu_engine.py's CASES with the same net and K)
    ('min', 1, False, False, 1e-4, 1e-3),
    ('min', 2, True, False, 1e-4, 2e-3),
    ('min', 2, False, True, 1e-4, 2e-3),
    ('omni', 1, False, False, 1e-4, 1e-3),
]


@pytest.mark.parametrize('net,K,per_step,fo,loss_floor,grad_floor', ORACLE_CASES)
def test_vector_call_vs_fp64_oracle(conv_form, net, K, per_step, fo, loss_floor, grad_floor):
    """Non-uniform steps (base * U(0.5, 1.5) per entry, block 1 frozen) on every operand form: loss, meta-gradient and lr_grad within
    max(floor, 2 x the fp32 oracle's own error), accuracy equal where the fp64 top-2 margin is clear."""
    _, mspec, theta, data, labels = _inputs(net)
    lr = _steps(net, K, per_step)
    eng = MetaEngine(mspec)
    loss, acc, grad, lr_grad, logits = _np(*eng.meta_batch_lr(theta, data, labels, SHOTS, K, torch.from_numpy(lr).cuda(), first_order=fo,
                                                              want_lr_grad=True, return_logits=True))
    l64, a64, g64, lg64, lo64, _ = _oracle(net, K, per_step, fo, True)
    l32, _, g32, lg32, _, _ = _oracle(net, K, per_step, fo, False)
    errs = dict(loss=np.abs(loss - l64) / np.abs(l64), grad=rel_err(grad, g64), lr_grad=rel_err(lr_grad, lg64))
    refs = dict(loss=np.abs(l32 - l64) / np.abs(l64), grad=rel_err(g32, g64), lr_grad=rel_err(lg32, lg64))
    report(f'inner_lr_oracle[{net} K{K} per_step{int(per_step)} fo{int(fo)}][{conv_form}]', loss_rel_err=float(errs['loss'].max()),
           ref_fp32_loss_rel_err=float(refs['loss'].max()), grad_rel_err=errs['grad'], ref_fp32_grad_rel_err=refs['grad'],
           lr_grad_rel_err=errs['lr_grad'], ref_fp32_lr_grad_rel_err=refs['lr_grad'])
    _held('loss', errs['loss'], refs['loss'], loss_floor)
    _held('grad', errs['grad'], refs['grad'], grad_floor)
    _held('lr_grad', errs['lr_grad'], refs['lr_grad'], grad_floor)
    assert lr_grad.shape == lr.shape
    for t in range(len(TASKS[net])):
        top2 = np.sort(lo64[t], axis=1)[:, -2:]
        clear = (top2[:, 1] - top2[:, 0]) > 1e-3 * max(1.0, np.abs(lo64[t]).max())
        assert np.array_equal(logits[t].argmax(axis=1)[clear], lo64[t].argmax(axis=1)[clear])
        if clear.all():
            assert acc[t] == a64[t]


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('per_step', [False, True])
def test_lr_grad_is_the_fold_of_the_traced_vectors(per_step):
    """lr_grad = -sum_t sum_k g[k] * lam_in[k] of the call's own trace.  One fp32 rounding per product and one of the fp64 sum of n terms
    (n = K T, or T per step): elementwise within (n + 2) 2^-24 sum |g lam| (+ n smallest-normal numbers: a product below that may lose
    bits).  Entries with step 0 keep theta_K == theta_0 bitwise, and their lr_grad is not all zero."""
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    T = data.shape[0]
    lr = _steps(net, K, per_step)
    eng = MetaEngine(mspec)
    tr = eng.set_trace(T, K)
    _, _, _, lr_grad, _ = eng.meta_batch_lr(theta, data, labels, SHOTS, K, torch.from_numpy(lr).cuda(), want_lr_grad=True)
    lr_grad, th, g, lam = _np(lr_grad, tr['theta'], tr['g'], tr['lam_in'])
    eng.set_trace(0)
    prod = g.astype(np.float64) * lam.astype(np.float64)                      # [K, T, P]
    want = -(prod.sum(1) if per_step else prod.sum((0, 1))[None])
    mag = np.abs(prod).sum(1) if per_step else np.abs(prod).sum((0, 1))[None]
    n = T if per_step else K * T
    bound = (n + 2) * 2.0 ** -24 * mag + n * 2.0 ** -126
    excess = np.abs(lr_grad - want) - bound
    report(f'inner_lr_trace[per_step{int(per_step)}]', worst_excess=float(excess.max()), rel=rel_err(lr_grad, want))
    assert np.all(excess <= 0)
    frozen = np.all(lr == 0, axis=0)
    assert frozen.any() and not frozen.all()
    assert np.array_equal(th[K][:, frozen], th[0][:, frozen]) and not np.array_equal(th[K][:, ~frozen], th[0][:, ~frozen])
    assert np.abs(lr_grad[:, frozen]).sum() > 0


# ---------------------------------------------------------------------------------------------------------------- 4
def test_reproducible_and_graph_replay_reads_the_step_sizes_from_the_device():
    """Eager, capture and two replays on the same buffers give identical bits; after the step sizes are overwritten IN PLACE the next
    (replayed) call equals a fresh eager engine on the new values."""
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    lr_a, lr_b = _steps(net, K, True), O.lr_vector(_specs(net)[0], 0.3, K, 9, frozen=('linear.',))
    vec = torch.from_numpy(lr_a).cuda()
    eng = MetaEngine(mspec)
    eng.set_graph(True)
    call = lambda e, v: _np(*e.meta_batch_lr(theta, data, labels, SHOTS, K, v, want_lr_grad=True, return_logits=True))
    first = call(eng, vec)
    for i in range(3):
        for a, b in zip(call(eng, vec), first):
            assert np.array_equal(a, b), i
    vec.copy_(torch.from_numpy(lr_b))
    replayed = call(eng, vec)
    fresh = MetaEngine(mspec)
    fresh.set_graph(False)
    for name, a, b in zip(('loss', 'acc', 'grad', 'lr_grad', 'logits'), replayed, call(fresh, torch.from_numpy(lr_b).cuda())):
        assert np.array_equal(a, b), name
    assert not np.array_equal(replayed[2], first[2])


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


def test_meta_batch_adapt_fills_model_and_step_size_gradients(monkeypatch):
    """InnerLR(per='tensor', learnable=True) through meta_batch_adapt: .backward() leaves the meta-gradient in the model's .grad and the
    per-tensor sums of lr_grad in the step sizes' .grad, both within the oracle rule (Mini-ImageNet K = 1 floors); the deferred outer
    backward gives the same gradient bits."""
    net, K = 'min', 1
    spec, _, _, data, labels = _inputs(net)
    model, theta = _model(net)
    names = [n for n, _ in model.named_parameters()]
    init = torch.from_numpy(0.5 * (0.5 + synthetic.hash_uniform(21, (1, len(names))))).float()
    got = {}
    for deferred in (False, True):
        monkeypatch.setattr(cf_vision, 'DEFERRED_OUTER_BACKWARD', deferred)
        il = cf.InnerLR(model, init, per='tensor', learnable=True, frozen=('base.0.',))
        maml = cf.MAML(model, lr=il)
        model.zero_grad()
        total, losses, accs = cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS)
        total.backward()
        got[deferred] = (_grads(model.parameters()), il.values.grad.cpu().numpy().copy(), _np(losses)[0])
    # deferred: the gradients come from the same full call, bit for bit; its losses come from the evaluation-only call, which agrees with the
    # full call's forward to rounding (test_gpu_engine.py::test_eval_only_and_batching_equivalence: rtol 1e-6)
    assert np.array_equal(got[False][0], got[True][0]) and np.array_equal(got[False][1], got[True][1])
    assert np.allclose(got[False][2], got[True][2], rtol=1e-6)
    grad, vgrad, loss = got[False]
    flat = il.flat().detach().cpu().numpy()
    res = {}
    for fp64 in (True, False):
        dtype = torch.float64 if fp64 else torch.float32
        datas, lbls = task_tensors(net, TASKS[net], WAYS, SHOTS, dtype)
        l, _, g, lg, _, _ = O.meta_batch(theta, spec, datas, lbls, K, SHOTS, WAYS, flat, False, dtype)
        sums, off = [], 0
        for _, p in model.named_parameters():                     # a per-tensor step receives the sum of its entries' gradients
            sums.append(lg[0, off:off + p.numel()].sum())
            off += p.numel()
        res[fp64] = (l, g, np.array(sums) * (flat[0, np.cumsum([0] + [p.numel() for p in model.parameters()][:-1])] != 0))
    (l64, g64, v64), (l32, g32, v32) = res[True], res[False]
    errs = (np.abs(loss - l64) / np.abs(l64), rel_err(grad, g64), rel_err(vgrad[0], v64))
    refs = (np.abs(l32 - l64) / np.abs(l64), rel_err(g32, g64), rel_err(v32, v64))
    report('inner_lr_python_surface', loss_rel_err=float(errs[0].max()), grad_rel_err=errs[1], step_grad_rel_err=errs[2],
           ref_fp32_loss_rel_err=float(refs[0].max()), ref_fp32_grad_rel_err=refs[1], ref_fp32_step_grad_rel_err=refs[2])
    for name, e, r, floor in zip(('loss', 'grad', 'step sizes'), errs, refs, (1e-4, 1e-3, 1e-3)):
        _held(name, e, r, floor)
    assert np.all(vgrad[0, :4] == 0) and np.abs(vgrad[0, 4:]).sum() > 0          # frozen block 1: no gradient reaches the stored values


def test_allow_nograd_freezes_in_the_fused_call_and_in_evaluate():
    """allow_nograd=True with requires_grad=False on base.0.*: the loss and accuracy of frozen=('base.0.',), no .grad on those
    parameters; without allow_nograd they are adapted as before.  evaluate runs with such learners."""
    net, K = 'min', 2
    _, _, _, data, labels = _inputs(net)
    model, _ = _model(net)
    for name, p in model.named_parameters():
        p.requires_grad_(not name.startswith('base.0.'))
    outs = {}
    for tag, maml in (('nograd', cf.MAML(model, lr=0.4, allow_nograd=True)),
                      ('frozen', cf.MAML(model, lr=cf.InnerLR(model, 0.4, per='scalar', frozen=('base.0.',)))),
                      ('plain', cf.MAML(model, lr=0.4))):
        model.zero_grad()
        total, losses, accs = cf.meta_batch_adapt(maml.clone(), data, labels, K, SHOTS, WAYS)
        total.backward()
        outs[tag] = _np(losses, accs) + (_grads(model.parameters()),)
        for name, p in model.named_parameters():
            assert (p.grad is None) == name.startswith('base.0.'), (tag, name)
    for a, b in zip(outs['nograd'], outs['frozen']):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs['nograd'][0], outs['plain'][0])
    from exploring_meta_amd.vision.maml_vision import SyntheticTasks
    p = dict(meta_batch_size=2, adapt_steps=K, shots=SHOTS, ways=WAYS)
    maml = cf.MAML(model, lr=0.4, allow_nograd=True)
    acc = cf.evaluate(p, SyntheticTasks(net, WAYS, SHOTS, 0), maml, torch.nn.CrossEntropyLoss(), torch.device('cuda'))
    with torch.no_grad():                                          # the same two tasks, adapted directly
        _, _, accs = cf.meta_batch_adapt(maml.clone(), data[:2].contiguous(), labels[:2].contiguous(), K, SHOTS, WAYS)
    assert acc == accs.mean().item()


@pytest.mark.parametrize('K,per_step', [(1, False), (2, True)])
def test_stepwise_learner_reaches_the_same_fast_weights(K, per_step):
    """learner.adapt with an InnerLR (theta - lr_flat * g, one row per step): the oracle's adapted weights under the bars of
    test_gpu_learner.py::test_stepwise_adapt_matches_oracle_and_fused (1e-4 after one step, 5e-3 after two), frozen entries untouched."""
    net = 'min'
    model, _ = _model(net)
    lr = _steps(net, K, per_step)
    il = cf.InnerLR(model, torch.from_numpy(lr), per='parameter', steps=lr.shape[0])
    learner = cf.MAML(model, lr=il).clone()
    datas, lbls = task_tensors(net, TASKS[net][:1], WAYS, SHOTS)
    ad, al, _, _ = R.prepare_batch(datas[0], lbls[0], SHOTS, WAYS)
    ad, al = ad.float().cuda(), al.cuda()
    loss = torch.nn.CrossEntropyLoss()
    for _ in range(K):
        learner.adapt(loss(learner(ad), al))
    fast = learner.fast_weights().detach().cpu().numpy()
    want = _oracle(net, K, per_step, False, True)[5][0]
    e = rel_err(fast, want)
    report(f'inner_lr_stepwise[K{K}]', fast_weights_rel=e)
    assert e < (1e-4 if K == 1 else 5e-3)
    frozen = np.all(lr == 0, axis=0)
    assert np.array_equal(fast[frozen], model.flat_parameters().detach().cpu().numpy()[frozen])
    if per_step:
        with pytest.raises(RuntimeError, match='step sizes for 2 inner steps'):
            learner.adapt(loss(learner(ad), al))


# ---------------------------------------------------------------------------------------------------------------- 6
def test_argument_errors_come_before_any_launch():
    net, K = 'min', 2
    _, mspec, theta, data, labels = _inputs(net)
    eng = MetaEngine(mspec)
    P = eng.param_count
    eng.profile(True)
    ok = torch.full((1, P), 0.4, device='cuda')
    with pytest.raises(_lib.MiError, match='lr_vec has shape'):
        eng.meta_batch_lr(theta, data, labels, SHOTS, K, ok[:, :-1].contiguous())
    with pytest.raises(_lib.MiError, match='lr_steps = 3'):
        eng.meta_batch_lr(theta, data, labels, SHOTS, K, torch.full((3, P), 0.4, device='cuda'))
    with pytest.raises(_lib.MiError, match='lr_grad_out given but grad_tasks = 0'):
        eng.meta_batch_lr(theta, data, labels, SHOTS, K, ok, grad_tasks=0, want_lr_grad=True)
    # the library's own checks, reached without the wrapper's
    import ctypes as C
    ws = eng._workspace(eng.workspace_bytes(3, SHOTS, K, True) + (1 << 20))
    out = torch.empty(P + 6, device='cuda')
    args = lambda vec, steps, lrg, gt: (eng._h, None, theta.data_ptr(), data.data_ptr(), labels.data_ptr(), 3, gt, WAYS, SHOTS, K, vec, steps, 1,
                                        out[P:].data_ptr(), out[P + 3:].data_ptr(), out.data_ptr(), lrg, None, ws.data_ptr(), ws.numel())
    for a, text in ((args(ok.data_ptr(), 3, None, 3), 'lr_steps = 3 must be 1 or adapt_steps = 2'), (args(None, 1, None, 3), 'lr_vec is NULL'),
                    (args(ok.data_ptr(), 1, ok.data_ptr(), 0), 'lr_grad_out given but grad_tasks = 0')):
        assert eng.lib.mi_meta_batch_maml_lr(*a) == -1
        assert text in eng.lib.mi_last_error(eng._h).decode()
    assert eng.profile_collect() == {}
    eng.profile(False)


# ---------------------------------------------------------------------------------------------------------------- 7
def _census(eng, fn):
    eng.profile(True)
    fn()
    torch.cuda.synchronize()
    c = {f'{op}/{layer}': int(n) for (op, layer), (_, n) in eng.profile_collect().items()}
    eng.profile(False)
    return c


@pytest.mark.parametrize('fused_tail', [1, 0])
def test_launch_make_up(fused_tail):
    """The vector call makes the scalar call's launches + 1 (the step sizes into engine layout: misc/1) + 1 with lr_grad (fold and scatter:
    misc/3); without the one-launch advance a second-order call adds per inner step 1 (the direction: misc/2) + 1 with lr_grad (the
    products).  The same at T = 1 and T = 3."""
    net, K = 'min', 2
    diffs = []
    for tasks in ([0], [0, 1, 2]):
        _, mspec, theta, data, labels = _inputs(net, tasks)
        eng = MetaEngine(mspec)
        eng.set_fused_tail(fused_tail)
        vec = torch.from_numpy(_steps(net, K, True)).cuda()
        for fo in (False, True):
            base = _census(eng, lambda: eng.meta_batch(theta, data, labels, SHOTS, K, 0.4, first_order=fo))
            for want in (False, True):
                got = _census(eng, lambda: eng.meta_batch_lr(theta, data, labels, SHOTS, K, vec, first_order=fo, want_lr_grad=want))
                diff = {k: got.get(k, 0) - base.get(k, 0) for k in set(got) | set(base) if got.get(k, 0) != base.get(k, 0)}
                extra = {'misc/1': 1}
                if want:
                    extra['misc/3'] = 1
                if not fused_tail and not fo:
                    extra['misc/2'] = K * (2 if want else 1)
                assert diff == extra, (tasks, fo, want, diff)
                diffs.append(diff)
    assert diffs[:4] == diffs[4:]
