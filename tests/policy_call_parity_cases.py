"""The calls behind tests/golden/policy_call_parent.npz, shared by tools/record_policy_call_parity.py (which runs them on the commit BEFORE
the policy / TRPO calls got one step descriptor per layer) and tests/test_gpu_policy_call_parity.py (which runs them on the code under
test): every `PolicyEngine` call that takes an inner-loop step, in its scalar form and in its table form, the workspace sizes and the
workspace's contents after a call.

A case is a function that returns lines `<variant> <quantity>=<hex> ...`, one per call it makes: a quantity of at most 16 values is there
with the hex of its bytes, the larger ones of a call (gradients, theta_out, products) go in order into one SHA-256 (`big=`).  Every line is
expected bit for bit.  Inputs are rebuilt from seeds (policy_lr_oracle.random_inputs / lr_vector, trpo_lr_oracle.make_case / directions);
the `inputs/*` cases hold their digests, so that a generator that drifted fails there and under that name."""
import ctypes as C
import functools
import hashlib
import os
from collections import OrderedDict

import numpy as np
import torch

import policy_lr_oracle as PO
import trpo_lr_oracle as TO
from exploring_meta_amd import _lib
from exploring_meta_amd import core_functions as cf
from exploring_meta_amd.core_functions.rl import _SurrogateContext
from exploring_meta_amd.engine import PolicyEngine, _ptr, _stream

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'policy_call_parent.npz')
LR = 0.1                                                # no power of two: d (.) (H x) and H (d (.) x) round differently
COUNTS = [(37, 20, 1), (25, 33, 39), (31, 1, 38)]       # test_gpu_policy_lr.ODD: ragged, one task with a single valid row
POLICIES = {'std': (2, 2, (100, 100), 'relu'), 'odd': (3, 1, (19, 33), 'tanh')}          # odd: P = 771, no multiple of 256 or 4
KIND = {'a2c': 0, 'ppo': 1, 'dice': 2}


def _line(variant, **tensors):
    parts, big = [variant], hashlib.sha256()
    for name, t in tensors.items():
        if t is None:
            parts.append(f'{name}=None')
            continue
        a = np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t))
        if a.size > 16:
            big.update(f'{name} {a.dtype} {a.shape}'.encode() + a.tobytes())
            parts.append(f'{name}=big')
        else:
            parts.append(f'{name}={a.dtype}{list(a.shape)}:{a.tobytes().hex()}')
    return ' '.join(parts + ['big=' + big.hexdigest()])


def _f(x):
    return x.float().cuda().contiguous()


def _batch(b):
    return dict(states=_f(b['states']), actions=_f(b['actions']), adv=_f(b['adv']), done=_f(b['done']),
                count=b['count'].to(torch.int32).cuda().contiguous())


@functools.lru_cache(maxsize=None)
def _policy_inputs(pol, T):
    """(engine, oracle net, theta, sup [2, T, 40, ..], qry) on the device; shared, read-only."""
    S, A, H, act = POLICIES[pol]
    inp = PO.random_inputs(S, A, H, 3, 40, COUNTS, seed=23)
    if T == 1:
        inp = PO.task_slice(inp, [1])                  # counts 20, 33, 1
    eng = PolicyEngine(S, A, H, activation=act)
    assert eng.param_count == inp['theta'].numel()
    return eng, PO.Oracle(S, A, H, act), _f(inp['theta']), _batch(inp['sup']), _batch(inp['qry'])


def _table(net, rows, frozen=()):
    """LR * U(0.5, 1.5) per entry, no two alike; ``frozen``: the tensors at exactly 0."""
    return _f(PO.lr_vector(net, LR, rows, 5, frozen=frozen))


def _ws_bytes(eng, fn, *args):
    b = C.c_size_t()
    assert getattr(eng.lib, fn)(eng._h, *args, C.byref(b)) == 0, (fn, args)
    return b.value


# --------------------------------------------------------------------------------------------------- meta-batch / update / adapt
def _meta_call(eng, net, theta, sup, qry, loss, form, head_only, first_order, with_grad, want_lr_grad=False, steps=2, frozen=()):
    """One meta_batch / meta_batch_lr call -> the outputs as _line takes them.  PPO: 2 epochs per batch, so step_new_old is 1, 0, 1, 0."""
    step_batch = [b for b in range(steps) for _ in range(2 if loss == 'ppo' else 1)]
    kw = dict(loss=loss, clip=0.1, head_only=head_only, first_order=first_order, with_grad=with_grad)
    if form == 'scalar':
        lt, th, grad = eng.meta_batch(theta, sup if steps else None, qry, step_batch, LR, **kw)
        return dict(loss=lt, theta_out=th, grad=grad)
    rows = 2 if form == 'rowsK' else 1
    lt, th, grad, lr_grad = eng.meta_batch_lr(theta, sup if steps else None, qry, step_batch, _table(net, rows, frozen),
                                              step_batch if form == 'rowsK' else None, want_lr_grad=want_lr_grad, **kw)
    return dict(loss=lt, theta_out=th, grad=grad, lr_grad=lr_grad)


def meta(pol, T, loss, form):
    eng, net, theta, sup, qry = _policy_inputs(pol, T)
    lines = []
    for head_only in (False, True):
        for fo, wg, lg in ((0, 1, 0), (1, 1, 0), (0, 0, 0), (0, 1, 1), (1, 1, 1)):
            if lg and form == 'scalar':
                continue
            out = _meta_call(eng, net, theta, sup, qry, loss, form, head_only, bool(fo), bool(wg), bool(lg))
            lines.append(_line(f'{"head" if head_only else "full"}/fo{fo}_wg{wg}_lg{lg}', **out))
    if loss == 'a2c':          # no update at all, and a table with an exactly-zero tensor
        lines.append(_line('steps0', **_meta_call(eng, net, theta, sup, qry, loss, form, False, False, True, form != 'scalar', steps=0)))
        if form != 'scalar':
            lines.append(_line('zero_tensor', **_meta_call(eng, net, theta, sup, qry, loss, form, False, False, True, True, frozen=('mean.0.',))))
    torch.cuda.synchronize()
    return lines


def _step_of(net, form):
    return LR if form == 'scalar' else _table(net, 2)[1]


def update(pol, loss, form):
    eng, net, theta, sup, _ = _policy_inputs(pol, 3)
    s0 = {k: v[0] for k, v in sup.items()}
    step, lines = _step_of(net, form), []
    for head_only in (False, True):
        for epochs in (1, 3):
            kw = dict(loss=loss, epochs=epochs, clip=0.1, done=s0['done'] if loss == 'dice' else None, head_only=head_only)
            out, losses = eng.update(theta, s0['states'], s0['actions'], s0['adv'], s0['count'], step, **kw)              # tstride 0
            lines.append(_line(f'{"head" if head_only else "full"}/shared_e{epochs}', theta_out=out, loss=losses))
            out2, losses2 = eng.update(out, s0['states'], s0['actions'], s0['adv'], s0['count'], step, **kw)              # tstride P
            lines.append(_line(f'{"head" if head_only else "full"}/per_task_e{epochs}', theta_out=out2, loss=losses2))
    torch.cuda.synchronize()
    return lines


def update_in_place(form):
    """theta_out is theta, through the library itself (PolicyEngine.update always allocates its output)."""
    eng, net, theta, sup, _ = _policy_inputs('std', 3)
    s0 = {k: v[0] for k, v in sup.items()}
    T, B, P = 3, s0['states'].shape[1], eng.param_count
    ws = torch.empty(_ws_bytes(eng, 'mi_policy_update_workspace_bytes', T, B), dtype=torch.uint8, device='cuda')
    lines = []
    for head_only in (0, 1):
        th = theta.expand(T, -1).contiguous()
        losses = torch.empty(T, 2, device='cuda')
        args = (eng._h, _stream(eng.device), _ptr(th), P, _ptr(s0['states']), _ptr(s0['actions']), _ptr(s0['adv']), _ptr(s0['count']), None, T, B,
                KIND['ppo'], 2, 0.1)
        tail = (head_only, _ptr(th), _ptr(losses), _ptr(ws), ws.numel())
        if form == 'scalar':
            assert eng.lib.mi_policy_update(*args, LR, *tail) == 0
        else:
            assert eng.lib.mi_policy_update_lr(*args, _ptr(_table(net, 2)[1].contiguous()), *tail) == 0
        lines.append(_line(f'{"head" if head_only else "full"}', theta_out=th, loss=losses))
    torch.cuda.synchronize()
    return lines


def adapt(form):
    eng, net, theta, sup, _ = _policy_inputs('std', 3)
    s0 = {k: v[0] for k, v in sup.items()}
    step, lines = _step_of(net, form), []
    for head_only in (False, True):
        out, loss = eng.adapt(theta, s0['states'], s0['actions'], s0['adv'], s0['count'], step, head_only=head_only)
        out2, loss2 = eng.adapt(out, s0['states'], s0['actions'], s0['adv'], s0['count'], step, head_only=head_only)
        lines += [_line(f'{"head" if head_only else "full"}/shared', theta_out=out, loss=loss),
                  _line(f'{"head" if head_only else "full"}/per_task', theta_out=out2, loss=loss2)]
    torch.cuda.synchronize()
    return lines


# --------------------------------------------------------------------------------------------------- TRPO
@functools.lru_cache(maxsize=None)
def _trpo_inputs(name):
    """(engine, theta, sup, qry, old_loc, old_scale, table [rows, P], rows of the K updates, two directions) of a trpo_lr_oracle case: the
    batches as meta_surrogate_loss assembles them."""
    c = TO.make_case(name)
    net = c['net']

    def policy(flat):
        p = cf.DiagNormalPolicy(net.S, net.A, list(net.H), activation=net.act_name).cuda()
        p.load_flat(_f(flat))
        return p
    pol = policy(c['theta'])
    ctx = _SurrogateContext(c['replays'], [policy(o) for o in c['olds']], pol, cf.LinearValue(net.S, net.A), c['params'])
    vs = [_f(v) for v in TO.directions(net, c['theta'])]
    return ctx.engine, pol.flat(), ctx.sup, ctx.qry, ctx.old_loc, ctx.old_scale, _f(c['lr_vec']), list(c['rows']), vs


def _trpo_sequence(name, form):
    """surrogate without and with the gradient, fvp, kl_prepare without and with kl_grad, fvp_general: (variant, outputs) per call."""
    eng, theta, sup, qry, old_loc, old_scale, table, rows, vs = _trpo_inputs(name)
    if form == 'scalar':
        lr, kw = LR, {}
    elif form == 'rows1':
        lr, kw = table[:1].contiguous(), {}
    else:
        lr, kw = table, dict(step_lr_row=rows)
    loss, kl, grad = eng.surrogate(theta, sup, qry, old_loc, old_scale, lr, False, **kw)
    yield 'surrogate', dict(loss=loss, kl=kl, grad=grad)
    loss, kl, grad = eng.surrogate(theta, sup, qry, old_loc, old_scale, lr, True, **kw)
    yield 'surrogate_grad', dict(loss=loss, kl=kl, grad=grad)
    for i, v in enumerate(vs):
        yield f'fvp{i}', dict(product=eng.fvp(sup, qry, lr, 1e-5, v, **kw))
    yield 'kl_prepare', dict(kl_grad=eng.kl_prepare(sup, qry, old_loc, old_scale, lr, False, **kw))
    yield 'kl_prepare_grad', dict(kl_grad=eng.kl_prepare(sup, qry, old_loc, old_scale, lr, True, **kw))
    for i, v in enumerate(vs):
        yield f'fvp_general{i}', dict(product=eng.fvp_general(sup, qry, old_scale, lr, 1e-5, v, **kw))


def trpo(name, form, fused=1):
    lib = _lib.load()
    lib.mi_policy_set_fused_fvp(fused)
    try:
        lines = [_line(variant, **out) for variant, out in _trpo_sequence(name, form)]
        torch.cuda.synchronize()
    finally:
        lib.mi_policy_set_fused_fvp(1)
    return lines


# --------------------------------------------------------------------------------------------------- sizes, layout, inputs
def sizes():
    """Every workspace size of the shapes above."""
    lines = []
    for pol, T in (('std', 3), ('odd', 1), ('odd', 3)):
        eng = _policy_inputs(pol, T)[0]
        B, v = 40, OrderedDict()
        v['meta'] = [_ws_bytes(eng, 'mi_policy_meta_workspace_bytes', T, B, K, NB, so) for K, NB in ((0, 0), (2, 2), (4, 2)) for so in (0, 1)]
        v['meta_lr'] = [_ws_bytes(eng, 'mi_policy_meta_lr_workspace_bytes', T, B, K, NB, so, rows, want)
                        for K, NB in ((0, 0), (2, 2), (4, 2)) for so in (0, 1) for rows in (1, 2) for want in (0, 1)]
        v['update'] = [_ws_bytes(eng, 'mi_policy_update_workspace_bytes', T, B)]
        v['learner'] = [_ws_bytes(eng, 'mi_policy_learner_workspace_bytes', T, B)]
        lines.append(_line(f'{pol}/T{T}', **{k: np.array(x, dtype=np.int64) for k, x in v.items()}))
    for name in ('relu_k1', 'tanh_k1', 'relu_k2'):
        eng, _, sup, _, _, _, _, _, _ = _trpo_inputs(name)
        K, T, B = sup['states'].shape[:3]
        v = OrderedDict()
        v['steps'] = [_ws_bytes(eng, 'mi_trpo_steps_workspace_bytes', T, B, K)]
        v['steps_lr'] = [_ws_bytes(eng, 'mi_trpo_steps_lr_workspace_bytes', T, B, K, rows) for rows in (1, K + 1)]
        v['general'] = [_ws_bytes(eng, 'mi_trpo_general_steps_workspace_bytes', T, B, K)]
        v['general_lr'] = [_ws_bytes(eng, 'mi_trpo_general_steps_lr_workspace_bytes', T, B, K, rows) for rows in (1, K + 1)]
        lines.append(_line(name, **{k: np.array(x, dtype=np.int64) for k, x in v.items()}))
    return lines


def layout(kind, form):
    """The workspace, as a digest, after calls that found it pre-sized and zeroed: every intermediate at its place.  Twice, so that what it
    records is known to repeat.  meta: the second-order meta-batch (table form: with want_lr_grad, g and prod behind the scalar plan);
    trpo: the general sequence at K = 2 (table form: dlam behind the general plan)."""
    digests = []
    for _ in range(2):
        if kind == 'meta':
            eng, net, theta, sup, qry = _policy_inputs('odd', 3)
            if form == 'scalar':
                n = _ws_bytes(eng, 'mi_policy_meta_workspace_bytes', 3, 40, 2, 2, 1)
            else:
                n = _ws_bytes(eng, 'mi_policy_meta_lr_workspace_bytes', 3, 40, 2, 2, 1, 2, 1)
            eng._ws = torch.zeros(n, dtype=torch.uint8, device='cuda')
            ws = eng._ws
            _meta_call(eng, net, theta, sup, qry, 'a2c', 'scalar' if form == 'scalar' else 'rowsK', False, False, True, True)
        else:
            eng, _, sup, _, _, _, table, _, _ = _trpo_inputs('relu_k2')
            K, T, B = sup['states'].shape[:3]
            if form == 'scalar':
                n = _ws_bytes(eng, 'mi_trpo_general_steps_workspace_bytes', T, B, K)
            else:
                n = _ws_bytes(eng, 'mi_trpo_general_steps_lr_workspace_bytes', T, B, K, table.shape[0])
            eng._ws = torch.zeros(n, dtype=torch.uint8, device='cuda')
            ws = eng._ws
            for _ in _trpo_sequence('relu_k2', form):
                pass
        torch.cuda.synchronize()
        assert eng._ws is ws and ws.numel() == n                    # the call took the buffer it found
        digests.append(_line('workspace', bytes=ws))
    assert digests[0] == digests[1]
    return digests[:1]


def inputs():
    lines = []
    for pol, T in (('std', 3), ('odd', 1), ('odd', 3)):
        _, net, theta, sup, qry = _policy_inputs(pol, T)
        flat = OrderedDict(theta=theta, **{f'sup_{k}': v for k, v in sup.items()}, **{f'qry_{k}': v for k, v in qry.items()})
        flat.update(table1=_table(net, 1), tableK=_table(net, 2), table_zero=_table(net, 2, ('mean.0.',)))
        lines.append(_line(f'{pol}/T{T}', **flat))
    for name in ('relu_k1', 'tanh_k1', 'relu_k2'):
        _, theta, sup, qry, old_loc, old_scale, table, rows, vs = _trpo_inputs(name)
        flat = OrderedDict(theta=theta, **{f'sup_{k}': v for k, v in sup.items()}, **{f'qry_{k}': v for k, v in qry.items()})
        flat.update(old_loc=old_loc, old_scale=old_scale, table=table, rows=np.array(rows), v0=vs[0], v1=vs[1])
        lines.append(_line(name, **flat))
    torch.cuda.synchronize()
    return lines


# case -> (function, its arguments)
CASES = OrderedDict([('inputs', (inputs, dict()))] + [
    (f'meta/{pol}/T{T}/{loss}/{form}', (meta, dict(pol=pol, T=T, loss=loss, form=form)))
    for pol, T in (('std', 3), ('odd', 1), ('odd', 3)) for loss in ('a2c', 'ppo', 'dice') for form in ('scalar', 'rows1', 'rowsK')] + [
    (f'update/{pol}/{loss}/{form}', (update, dict(pol=pol, loss=loss, form=form)))
    for pol in ('std', 'odd') for loss in ('a2c', 'ppo', 'dice') for form in ('scalar', 'row')] + [
    (f'update_in_place/{form}', (update_in_place, dict(form=form))) for form in ('scalar', 'row')] + [
    (f'adapt/{form}', (adapt, dict(form=form))) for form in ('scalar', 'row')] + [
    (f'trpo/{name}/{form}', (trpo, dict(name=name, form=form))) for name in ('relu_k1', 'tanh_k1') for form in ('scalar', 'rows1')] + [
    (f'trpo/relu_k1_per_layer/{form}', (trpo, dict(name='relu_k1', form=form, fused=0))) for form in ('scalar', 'rows1')] + [
    (f'trpo/relu_k2/{form}', (trpo, dict(name='relu_k2', form=form))) for form in ('scalar', 'rows1', 'rowsK')] + [
    ('sizes', (sizes, dict()))] + [
    (f'layout/{kind}/{form}', (layout, dict(kind=kind, form=form))) for kind in ('meta', 'trpo') for form in ('scalar', 'table')])


def compute(only=''):
    """{'<case>': its lines as a bytes array} (what the recorder stores); only: the cases that start with it."""
    return OrderedDict((case, np.array(fn(**kw), dtype=np.bytes_)) for case, (fn, kw) in CASES.items() if case.startswith(only))
