"""The calls behind tests/golden/fused_call_parent.npz, shared by tools/record_fused_call_parity.py (which runs them on the commit BEFORE
the fused MAML / ANIL calls got one call descriptor per layer) and tests/test_gpu_fused_call_parity.py (which runs them on the code
under test): `meta_batch`, `meta_batch_lr`, `meta_batch_anil`, the step-wise learner, graph mode, the autograd layer, the workspace
sizes and the workspace's contents after a call.  5-way on the mini-ImageNet net, 1-shot unless said otherwise, tasks 0..2, K = 2.  Arrays of more than 64 values (gradients,
logits) are recorded as SHA-256 digests of their bytes, the others as they are: every quantity is expected bit for bit."""
import ctypes as C
import hashlib
import os
from collections import OrderedDict

import numpy as np
import torch

import inner_lr_oracle as O
import test_gpu_launch_census as census
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions import vision as cf_vision
from exploring_meta_amd.core_functions.anil import meta_batch_adapt_anil
from exploring_meta_amd.engine import MetaEngine, ModelSpec
from exploring_meta_amd.utils import synthetic
from helpers import hash_params
from oracle import vision_ref as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fused_call_parent.npz')
WAYS, TASKS, K, LR = 5, (0, 1, 2), 2, 0.4


def _rec(**tensors):
    """name -> array as recorded: None dropped, more than 64 values as '<name>_sha256'."""
    out = OrderedDict()
    for name, t in tensors.items():
        if t is None:
            continue
        a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
        if a.size > 64:
            out[name + '_sha256'] = np.asarray(hashlib.sha256(a.tobytes()).hexdigest() + f' {a.dtype} {a.shape}')
        else:
            out[name] = a
    return out


def _batch(shots=1):
    data, labels = synthetic.make_meta_batch('min', list(TASKS), WAYS, shots)
    return torch.from_numpy(data).cuda().contiguous(), torch.from_numpy(labels).cuda().contiguous()


def _theta():
    """The weights of tests/test_gpu_launch_census.py: the reference's initialisers."""
    shapes = R.param_shapes(R.mini_imagenet_spec(WAYS))
    return R.flatten_params(OrderedDict((k, torch.from_numpy(v)) for k, v in synthetic.ref_init_weights(shapes, 11).items())).float().cuda()


def _anil_theta():
    base = dict(kind='min', in_shape=(3, 84, 84), base=R.convbase_spec(64, 3, True))
    return torch.cat([R.flatten_params(hash_params(R.param_shapes(base, prefix_base='0.'), 13)),
                      R.flatten_params(hash_params({'weight': (WAYS, 1600), 'bias': (WAYS,)}, 17))]).float().cuda()


def _lr_vec(steps):
    """No power of two, no two entries alike: 0.4 * U(0.5, 1.5) per entry."""
    return torch.from_numpy(O.lr_vector(R.mini_imagenet_spec(WAYS), LR, steps, 5, frozen=())).cuda().contiguous()


def _engine(spec, switches):
    eng = MetaEngine(spec)
    for name, value in switches.items():
        getattr(eng, name)(value)
    return eng


def maml(shots=1, steps=K, switches=None, **kw):
    eng = _engine(ModelSpec.mini_imagenet(WAYS), switches or {})
    data, labels = _batch(shots)
    loss, acc, grad, logits = eng.meta_batch(_theta(), data, labels, shots, steps, LR, **kw)
    return _rec(loss=loss, acc=acc, grad=grad, logits=logits)


def maml_lr(lr_steps, switches=None, **kw):
    eng = _engine(ModelSpec.mini_imagenet(WAYS), switches or {})
    data, labels = _batch()
    loss, acc, grad, lr_grad, logits = eng.meta_batch_lr(_theta(), data, labels, 1, K, _lr_vec(lr_steps), **kw)
    return _rec(loss=loss, acc=acc, grad=grad, lr_grad=lr_grad, logits=logits)


def anil(**kw):
    eng = MetaEngine(ModelSpec.anil(WAYS))
    data, labels = _batch()
    loss, acc, grad, logits = eng.meta_batch_anil(_anil_theta(), data, labels, 1, K, LR, return_logits=True, **kw)
    return _rec(loss=loss, acc=acc, grad=grad, logits=logits)


def learner(name):
    """The step-wise learner cases of the launch census (forward with rep_layer, backward, hvp; shared and per-task theta)."""
    return _rec(**census.run_case(census.CASES[name])[1])


def graph(kind):
    """Graph mode on one engine: three calls in a row (eager, capture, replay), a call after theta's (and the step sizes') values
    changed in place, for the vector call one with the step sizes in another buffer, and one after set_fused_tail(0)."""
    eng = MetaEngine(ModelSpec.anil(WAYS) if kind == 'anil' else ModelSpec.mini_imagenet(WAYS))
    eng.set_graph(True)
    data, labels = _batch()
    theta = _anil_theta() if kind == 'anil' else _theta()
    lr_vec = _lr_vec(K) if kind == 'maml_lr' else None

    def call(lr=None):
        if kind == 'maml':
            loss, acc, grad, logits = eng.meta_batch(theta, data, labels, 1, K, LR)
            return _rec(loss=loss, acc=acc, grad=grad, logits=logits)
        if kind == 'anil':
            loss, acc, grad, logits = eng.meta_batch_anil(theta, data, labels, 1, K, LR, return_logits=True)
            return _rec(loss=loss, acc=acc, grad=grad, logits=logits)
        loss, acc, grad, lr_grad, logits = eng.meta_batch_lr(theta, data, labels, 1, K, lr_vec if lr is None else lr, want_lr_grad=True)
        return _rec(loss=loss, acc=acc, grad=grad, lr_grad=lr_grad, logits=logits)

    out = OrderedDict()
    for i in range(3):
        out.update((f'call{i}/{k}', v) for k, v in call().items())
    theta.mul_(1.01)
    if lr_vec is not None:
        lr_vec.mul_(0.9)
    out.update((f'moved/{k}', v) for k, v in call().items())
    if lr_vec is not None:
        other = (lr_vec * 1.1).contiguous()          # (lr_vec stays alive: the captured graph reads it)
        out.update((f'other_buffer/{k}', v) for k, v in call(other).items())
    eng.set_fused_tail(0)
    out.update((f'tail_off/{k}', v) for k, v in call().items())
    torch.cuda.synchronize()
    return out


def layout(kind):
    """The workspace, as a digest, after one call that found it zeroed: every intermediate at its place.  No entry point reports a plan's
    offsets in full (mi_debug_plan_offsets names ten, all in front of the partial buffers); this sees them all, twice, so that what it
    records is known to repeat."""
    eng = MetaEngine(ModelSpec.anil(WAYS) if kind == 'anil' else ModelSpec.mini_imagenet(WAYS))
    data, labels = _batch()
    T, b, digests = len(TASKS), C.c_size_t(), []
    if kind == 'anil':
        assert eng.lib.mi_anil_workspace_bytes(eng._h, T, WAYS, 1, K, C.byref(b)) == 0
    elif kind == 'maml_lr':
        assert eng.lib.mi_workspace_bytes_lr(eng._h, T, WAYS, 1, K, 1, K, 1, C.byref(b)) == 0
    else:
        b.value = eng.workspace_bytes(T, 1, K, True)
    for _ in range(2):
        eng._workspace(b.value).zero_()
        if kind == 'anil':
            eng.meta_batch_anil(_anil_theta(), data, labels, 1, K, LR)
        elif kind == 'maml_lr':
            eng.meta_batch_lr(_theta(), data, labels, 1, K, _lr_vec(K), want_lr_grad=True)
        else:
            eng.meta_batch(_theta(), data, labels, 1, K, LR)
        torch.cuda.synchronize()
        assert eng._ws.numel() >= b.value
        digests.append(_rec(workspace=eng._ws[:b.value]))
    assert str(digests[0]['workspace_sha256']) == str(digests[1]['workspace_sha256'])
    return digests[0]


def _model():
    model = cf.MiniImagenetCNN(WAYS)
    shapes = R.param_shapes(R.mini_imagenet_spec(WAYS))
    with torch.no_grad():
        init = synthetic.ref_init_weights(shapes, 11)
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(init[k]).float())
    return model.cuda()


def _grads(params):
    return torch.cat([p.grad.reshape(-1) for p in params])


def adapt(how, deferred=False):
    """`meta_batch_adapt` / `meta_batch_adapt_anil` and .backward(): the returns and what lands in .grad."""
    data, labels = _batch()
    was = cf_vision.DEFERRED_OUTER_BACKWARD
    cf_vision.DEFERRED_OUTER_BACKWARD = deferred
    try:
        if how == 'anil':
            base = dict(kind='min', in_shape=(3, 84, 84), base=R.convbase_spec(64, 3, True))
            tf, th = hash_params(R.param_shapes(base, prefix_base='0.'), 13), hash_params({'weight': (WAYS, 1600), 'bias': (WAYS,)}, 17)
            trunk, head = cf.ConvBase(output_size=64, channels=3, max_pool=True), torch.nn.Linear(1600, WAYS)
            with torch.no_grad():
                for k, p in trunk.named_parameters():
                    p.copy_(tf['0.' + k].float())
                head.weight.copy_(th['weight'].float())
                head.bias.copy_(th['bias'].float())
            features, learner_ = torch.nn.Sequential(trunk).cuda(), cf.MAML(head, lr=LR).cuda()
            total, losses, accs = meta_batch_adapt_anil(learner_.clone(), features, data, labels, K, 1, WAYS)
            total.backward()
            return _rec(loss_sum=total, loss=losses, acc=accs, grad=_grads(list(features.parameters()) + list(head.parameters())))
        model = _model()
        if how == 'scalar':
            maml_, il = cf.MAML(model, lr=LR), None
        else:
            names = [n for n, _ in model.named_parameters()]
            init = torch.from_numpy(LR * (0.5 + synthetic.hash_uniform(21, (K, len(names))))).float()
            il = cf.InnerLR(model, init, per='tensor', steps=K, learnable=True)
            maml_ = cf.MAML(model, lr=il)
        total, losses, accs = cf.meta_batch_adapt(maml_.clone(), data, labels, K, 1, WAYS)
        total.backward()
        return _rec(loss_sum=total, loss=losses, acc=accs, grad=_grads(model.parameters()), lr_grad=None if il is None else il.values.grad)
    finally:
        cf_vision.DEFERRED_OUTER_BACKWARD = was


def sizes(_=None):
    """Every workspace size of the shapes above, and mi_debug_plan_offsets' ten entries."""
    eng, an = MetaEngine(ModelSpec.mini_imagenet(WAYS)), MetaEngine(ModelSpec.anil(WAYS))
    T, b, out = len(TASKS), C.c_size_t(), OrderedDict()

    def q(e, fn, *args):
        assert getattr(e.lib, fn)(e._h, *args, C.byref(b)) == 0, (fn, args)
        return b.value

    shapes = [(1, K, 1), (1, K, 0), (1, 0, 1), (1, 0, 0), (5, K, 1), (5, K, 0)]          # (shots, adapt_steps, second_order)
    out['workspace_bytes'] = np.array([q(eng, 'mi_workspace_bytes', T, WAYS, s, k, so) for s, k, so in shapes], dtype=np.int64)
    out['workspace_bytes_lr'] = np.array([q(eng, 'mi_workspace_bytes_lr', T, WAYS, 1, K, so, steps, want)
                                          for so in (1, 0) for steps in (1, K) for want in (0, 1)], dtype=np.int64)
    out['anil_workspace_bytes'] = np.array([q(an, 'mi_anil_workspace_bytes', T, WAYS, 1, k) for k in (K, 0)], dtype=np.int64)
    out['forward_workspace_bytes'] = np.array([q(eng, 'mi_forward_workspace_bytes', 2, 5), q(eng, 'mi_forward_workspace_bytes', T, 25)], dtype=np.int64)
    out['learner_hvp_workspace_bytes'] = np.array([q(eng, 'mi_learner_hvp_workspace_bytes', 2, 5)], dtype=np.int64)
    offs = (C.c_size_t * 10)()
    rows = []
    for s, k, so in shapes:
        assert eng.lib.mi_debug_plan_offsets(eng._h, T, WAYS, s, k, so, offs) == 0
        rows.append(list(offs))
    out['plan_offsets'] = np.array(rows, dtype=np.int64)
    return out


# call -> (function, its arguments)
CALLS = OrderedDict([
    ('maml/second_order', (maml, dict())),
    ('maml/first_order', (maml, dict(first_order=True))),
    ('maml/grad_tasks_2', (maml, dict(grad_tasks=2))),
    ('maml/forward_only', (maml, dict(with_grad=False))),
    ('maml/K_0', (maml, dict(steps=0))),
    ('maml/logits', (maml, dict(return_logits=True))),
    ('maml/5_shot_fused_tail_0', (maml, dict(shots=5, switches=dict(set_fused_tail=0)))),
    ('maml_lr/steps_1', (maml_lr, dict(lr_steps=1))),
    ('maml_lr/steps_1_lr_grad', (maml_lr, dict(lr_steps=1, want_lr_grad=True))),
    ('maml_lr/steps_K', (maml_lr, dict(lr_steps=K))),
    ('maml_lr/steps_K_lr_grad', (maml_lr, dict(lr_steps=K, want_lr_grad=True, return_logits=True))),
    ('maml_lr/first_order_lr_grad', (maml_lr, dict(lr_steps=K, first_order=True, want_lr_grad=True))),
    ('maml_lr/grad_tasks_0', (maml_lr, dict(lr_steps=1, grad_tasks=0))),
    ('maml_lr/fused_tail_0_lr_grad', (maml_lr, dict(lr_steps=K, want_lr_grad=True, return_logits=True, switches=dict(set_fused_tail=0)))),
    ('anil/second_order', (anil, dict())),
    ('anil/first_order', (anil, dict(first_order=True))),
    ('anil/forward_only', (anil, dict(with_grad=False))),
] + [(f'learner/{how}_{call}', (learner, dict(name=f'learner_{how}_{call}')))
     for how in ('shared_theta', 'per_task_theta') for call in ('forward', 'backward', 'hvp')] + [
    ('graph/maml', (graph, dict(kind='maml'))),
    ('graph/maml_lr', (graph, dict(kind='maml_lr'))),
    ('graph/anil', (graph, dict(kind='anil'))),
    ('adapt/scalar', (adapt, dict(how='scalar'))),
    ('adapt/inner_lr', (adapt, dict(how='inner_lr'))),
    ('adapt/anil', (adapt, dict(how='anil'))),
    ('adapt_deferred/scalar', (adapt, dict(how='scalar', deferred=True))),
    ('adapt_deferred/inner_lr', (adapt, dict(how='inner_lr', deferred=True))),
    ('sizes', (sizes, dict())),
    ('layout/maml', (layout, dict(kind='maml'))),
    ('layout/maml_lr', (layout, dict(kind='maml_lr'))),
    ('layout/anil', (layout, dict(kind='anil'))),
])

# Where a quantity's expected value is another call's fixture: the eager, capture and replay calls of graph mode give what the eager call
# gave, and the deferred outer backward what the undeferred run gave.
_GRAPH_EAGER = {'graph/maml': 'maml/second_order', 'graph/maml_lr': 'maml_lr/steps_K_lr_grad', 'graph/anil': 'anil/second_order'}


def fixture_key(call, quantity):
    if call in _GRAPH_EAGER and quantity.startswith('call'):
        return f'{_GRAPH_EAGER[call]}/{quantity.split("/", 1)[1]}'
    if call.startswith('adapt_deferred/'):
        return f'adapt/{call.split("/", 1)[1]}/{quantity}'
    return f'{call}/{quantity}'


def compute(only=''):
    """Every quantity under its own name, {'<call>/<quantity>': array} (what the recorder stores); only: the calls that start with it."""
    arrays = OrderedDict()
    for call, (fn, kw) in CALLS.items():
        if call.startswith(only):
            arrays.update((f'{call}/{k}', v) for k, v in fn(**kw).items())
    return arrays
