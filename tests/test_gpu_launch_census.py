"""Launch census: WHICH launches every engine entry point makes, per (op name, layer), against tests/launch_census.json.

The equivalence tests compare results; this one pins the launch sequence's make-up, so that a change of the engine's host code (csrc/engine.hip)
that adds, drops or relabels a launch shows even where the results survive it.  The table holds counts only and was recorded once, with
tools/record_launch_census.py, from a build of the commit BEFORE the primal and tangent sweeps were folded into one (MI_MAML_LIB selects the
library), the rows of the step-size-vector call (maml_lr_*) from the commit before the fused calls got one call descriptor: never from the
code under test.  Counts do not depend on the device's size.  Profiling runs every call eagerly (no graph replay)."""
import json
import os
from collections import OrderedDict

import pytest
import torch

from exploring_meta_amd.engine import MetaEngine, ModelSpec
from exploring_meta_amd.utils import synthetic
from oracle import vision_ref as R
from helpers import hash_params, model_params

pytestmark = pytest.mark.gpu

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'launch_census.json')


def _maml(net='min', shots=1, K=2, tasks=(0, 1, 2), first_order=False, with_grad=True, grad_tasks=None, **switches):
    return dict(kind='maml', net=net, shots=shots, K=K, tasks=list(tasks), first_order=first_order, with_grad=with_grad,
                grad_tasks=grad_tasks, switches=switches)


def _maml_lr(lr_steps=1, want_lr_grad=False, first_order=False, **switches):
    """The step-size-vector call on the default MAML case's batch: 0.4 * U(0.5, 1.5) per entry."""
    return dict(kind='maml_lr', lr_steps=lr_steps, want_lr_grad=want_lr_grad, first_order=first_order, switches=switches)


# The smallest cases that reach every branch of trunk_forward / trunk_backward (5-way throughout).
CASES = OrderedDict([
    # default MAML: mini-ImageNet net, 1-shot, K = 2, tasks 0..2
    ('maml_fused_block1_1', _maml(set_fused_block1=1)),
    ('maml_fused_block1_2', _maml(set_fused_block1=2)),
    ('maml_fused_block1_0', _maml(set_fused_block1=0)),
    ('maml_first_order', _maml(first_order=True, set_fused_block1=1)),
    ('maml_grad_tasks_2_of_3', _maml(grad_tasks=2, set_fused_block1=1)),
    ('maml_forward_only', _maml(with_grad=False, set_fused_block1=1)),
    # one switch off at a time: 5-shot, K = 2, tasks 3, 4
    ('switches_default', _maml(shots=5, tasks=(3, 4))),
    ('switches_fused_tail_0', _maml(shots=5, tasks=(3, 4), set_fused_tail=0)),
    ('switches_fused_last_block_0', _maml(shots=5, tasks=(3, 4), set_fused_last_block=0)),
    ('switches_fused_finalize_0', _maml(shots=5, tasks=(3, 4), set_fused_finalize=0)),
    ('switches_fused_block1_reduce_0', _maml(shots=5, tasks=(3, 4), set_fused_block1_reduce=0)),
    ('switches_overlap_0', _maml(shots=5, tasks=(3, 4), set_overlap=False)),
    # Omniglot net: stride 2, mean-pooled head
    ('omniglot', _maml(net='omni', K=1, tasks=(0, 1))),
    ('anil', dict(kind='anil', shots=1, K=2, tasks=[0, 1])),
    ('maml_lr_default', _maml_lr()),
    ('maml_lr_grad', _maml_lr(want_lr_grad=True)),
    ('maml_lr_per_step_grad', _maml_lr(lr_steps=2, want_lr_grad=True)),
    ('maml_lr_fused_tail_0_grad', _maml_lr(want_lr_grad=True, set_fused_tail=0)),
    ('maml_lr_first_order_grad', _maml_lr(want_lr_grad=True, first_order=True)),
] + [(f'learner_{how}_{call}', dict(kind='learner', call=call, per_task_theta=how == 'per_task_theta'))
     for how in ('shared_theta', 'per_task_theta') for call in ('forward', 'backward', 'hvp')])

WAYS = 5


def run_case(case, trace=False):
    """One case on a fresh engine with profiling on.  Returns ({'op name/layer': launches}, {name: output tensor}); trace: also the
    set_trace vectors of a second-order MAML call whose tasks all take the backward half."""
    out = OrderedDict()
    if case['kind'] == 'maml':
        omni = case['net'] == 'omni'
        ref_spec = R.omniglot_spec(WAYS) if omni else R.mini_imagenet_spec(WAYS)
        eng = MetaEngine(ModelSpec.omniglot(WAYS) if omni else ModelSpec.mini_imagenet(WAYS))
        for name, value in case['switches'].items():
            getattr(eng, name)(value)
        theta = R.flatten_params(OrderedDict((k, torch.from_numpy(v)) for k, v in
                                             synthetic.ref_init_weights(R.param_shapes(ref_spec), 11).items())).float().cuda()
        data, labels = synthetic.make_meta_batch(case['net'], case['tasks'], WAYS, case['shots'])
        data, labels = torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda()
        T, K = len(case['tasks']), case['K']
        traced = trace and case['with_grad'] and not case['first_order'] and case['grad_tasks'] in (None, T)
        tr = eng.set_trace(T, K) if traced else None
        eng.profile(True)
        loss, acc, grad, logits = eng.meta_batch(theta, data, labels, case['shots'], K, 0.4, first_order=case['first_order'],
                                                 with_grad=case['with_grad'], return_logits=True, grad_tasks=case['grad_tasks'])
        out.update(loss=loss, acc=acc, grad=grad, logits=logits)
        if tr:
            out.update(('trace_' + k, v) for k, v in tr.items())
    elif case['kind'] == 'maml_lr':   # mini-ImageNet net, 1-shot, K = 2, tasks 0..2
        eng = MetaEngine(ModelSpec.mini_imagenet(WAYS))
        for name, value in case['switches'].items():
            getattr(eng, name)(value)
        theta = R.flatten_params(OrderedDict((k, torch.from_numpy(v)) for k, v in
                                             synthetic.ref_init_weights(R.param_shapes(R.mini_imagenet_spec(WAYS)), 11).items())).float().cuda()
        data, labels = synthetic.make_meta_batch('min', [0, 1, 2], WAYS, 1)
        lr_vec = torch.from_numpy(0.4 * (0.5 + synthetic.hash_uniform(5, (case['lr_steps'], eng.param_count)))).float().cuda()
        eng.profile(True)
        loss, acc, grad, lr_grad, logits = eng.meta_batch_lr(theta, torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda(), 1, 2, lr_vec,
                                                             first_order=case['first_order'], want_lr_grad=case['want_lr_grad'],
                                                             return_logits=True)
        out.update(loss=loss, acc=acc, grad=grad, lr_grad=lr_grad, logits=logits)
    elif case['kind'] == 'anil':
        eng = MetaEngine(ModelSpec.anil(WAYS))
        base = dict(kind='min', in_shape=(3, 84, 84), base=R.convbase_spec(64, 3, True))
        theta = torch.cat([R.flatten_params(hash_params(R.param_shapes(base, prefix_base='0.'), 13)),
                           R.flatten_params(hash_params({'weight': (WAYS, 1600), 'bias': (WAYS,)}, 17))]).float().cuda()
        data, labels = synthetic.make_meta_batch('min', case['tasks'], WAYS, case['shots'])
        eng.profile(True)
        loss, acc, grad, logits = eng.meta_batch_anil(theta, torch.from_numpy(data).cuda(), torch.from_numpy(labels).cuda(), case['shots'],
                                                      case['K'], 0.4, return_logits=True)
        out.update(loss=loss, acc=acc, grad=grad, logits=logits)
    else:   # the step-wise learner: 2 tasks x 5 images of the mini-ImageNet net
        eng = MetaEngine(ModelSpec.mini_imagenet(WAYS))
        theta = R.flatten_params(model_params(R.mini_imagenet_spec(WAYS), 11)).float().cuda()
        if case['per_task_theta']:
            theta = torch.stack([theta, theta * 1.01])
        data, _ = synthetic.make_meta_batch('min', [0, 1], WAYS, 1)
        x = torch.from_numpy(data[:, :5]).contiguous().cuda()
        dl = torch.from_numpy(synthetic.hash_normalish(5, (2, 5, WAYS))).float().cuda()
        v = torch.from_numpy(synthetic.hash_normalish(6, tuple(theta.reshape(-1, eng.param_count).shape))).float().cuda()
        eng.profile(True)
        if case['call'] == 'forward':
            out['logits'], out['rep'] = eng.learner_forward(theta, x, rep_layer=2)
        elif case['call'] == 'backward':
            out['grad'] = eng.learner_backward(theta, x, dl)
        else:
            out['grad_theta'], out['logits_dot'] = eng.learner_hvp(theta, x, dl, v)
    census = {f'{op}/{layer}': int(launches) for (op, layer), (_, launches) in sorted(eng.profile_collect().items())}
    eng.profile(False)
    return census, OrderedDict((k, t) for k, t in out.items() if t is not None)


@pytest.fixture(scope='module')
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_covers_exactly_these_cases(table):
    assert sorted(table) == sorted(CASES)


@pytest.mark.parametrize('name', list(CASES))
def test_launch_census(table, name):
    census, _ = run_case(CASES[name])
    assert census == table[name], {k: (census.get(k), table[name].get(k)) for k in sorted(set(census) | set(table[name]))
                                   if census.get(k) != table[name].get(k)}
