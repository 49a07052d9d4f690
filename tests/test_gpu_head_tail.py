"""The last stage of every pass at the limits of its domain: the classifier head (csrc/head.hip, csrc/head_bodies.h: primal, tangent, the
fixed-cotangent and fd == NULL modes, the spatial mean) and the one-launch tail (csrc/tail.hip), each against the fp64 restatement in
oracle/kernels_ref.py -- at the widths where head_row_at / head_grads_chunk change path (ways 1, 2, 8 | 9, 33, 64; feat % 4 != 0; one and two
512-feature rounds; n <= 32 < n), with per-task strides that put some tasks on the 16-byte path and others on the scalar one, at the largest
n * ways that fits the gradient launch's LDS, and on every limit of tail_supported.  The tail is also held bit for bit to the separate launches
(mi_bn_relu_pool, mi_head_fwd_bwd, mi_bn_tangent_fwd, mi_head_tangent) at the same shapes.

Bars: the primal head's are test_gpu_kernels.py::test_head_fwd_bwd's (loss 2e-6 abs, logits 5e-6 abs, dWl / dbl / df 5e-6 rel), the BatchNorm and
pooling part's are test_bn_relu_pool_fwd_bwd's (5e-6), tangent quantities take test_bn_tangent_fwd_bwd's (forward tangents 1e-5 abs, gradient
tangents 5e-6 rel).  prob is held to the logits bar (|d softmax| <= |d logits| / 2) and dlogits to the gradients' 5e-6 rel.  Only the large-logit
and the n * ways-limit cases may instead take 4x the error of the SAME fp64 reference code run in fp32 on the same inputs (`_yardstick`), where
that is larger than the bar: both figures go through report()."""
import ctypes as C

import numpy as np
import pytest
import torch

from exploring_meta_amd import _lib
from exploring_meta_amd.utils import synthetic
from oracle import kernels_ref as KR
from gpu_utils import dev, ptr, stream, rel_err, max_err, report

pytestmark = pytest.mark.gpu

NAN = float('nan')
HEAD_LDS_LIMIT = 160 * 1024          # include/mi_maml.h, comment on mi_model_desc::ways


@pytest.fixture(scope='module')
def lib():
    return _lib.load()


def _rand(seed, shape, lo=-1.0, hi=1.0):
    return (synthetic.hash_uniform(seed, shape) * (hi - lo) + lo).astype(np.float32)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def _nan(*shape):
    return torch.full(shape, NAN, device='cuda')


def _at(buf, off):
    return C.c_void_p(buf.data_ptr() + 4 * off)


def _np(t):
    return t.detach().cpu().numpy()


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _labels(T, n, ways):
    """Class 0 and class ways - 1 first, then inwards; task t starts t places further on (so n == 1 still sees both ends over the tasks)."""
    k = np.arange(n)[None, :] + np.arange(T)[:, None]
    return np.where(k % 2 == 0, (k // 2) % ways, ways - 1 - (k // 2) % ways).astype(np.int32)


def _head_lds(n, ways, tangent):
    return ((2 if tangent else 1) * n * ways + 3 * 8 * 64) * 4


def _largest_n(ways, tangent):
    return (HEAD_LDS_LIMIT // 4 - 3 * 8 * 64) // ((2 if tangent else 1) * ways)


# ------------------------------------------------------------------------------------------------------------ head: inputs, runs, references
class HeadCase:
    """Inputs of one head case: T tasks with distinct parameters; theta / direction strides = 2 (mod 4) floats, so that tasks 0 and 2 start on a
    16-byte boundary and task 1 does not (the vector path of head_row_at needs the boundary); the gradient stride is odd."""

    def __init__(self, T, n, feat, ways, seed=40, wscale=0.1):
        self.T, self.n, self.feat, self.ways = T, n, feat, ways
        self.f = _rand(seed, (T, n, feat), 0.0, 1.5)
        self.wl = _rand(seed + 1, (T, ways, feat), -wscale, wscale)
        self.bl = _rand(seed + 2, (T, ways), -0.1, 0.1)
        self.fd = _rand(seed + 3, (T, n, feat), -1.0, 1.0)
        self.wld = _rand(seed + 4, (T, ways, feat), -0.05, 0.05)
        self.bld = _rand(seed + 5, (T, ways), -0.1, 0.1)
        self.y = _labels(T, n, ways)

    def strides(self):
        size = self.ways * self.feat + self.ways
        ps = size + 1
        while ps % 4 != 2:
            ps += 1
        gs = size + 3
        gs += 1 - gs % 2
        return ps, ps + 4, gs

    def pack(self):
        T, wf = self.T, self.ways * self.feat
        ps, vs, gs = self.strides()
        pb, vb = np.zeros((T, ps), np.float32), np.zeros((T, vs), np.float32)
        pb[:, :wf], pb[:, wf:wf + self.ways] = self.wl.reshape(T, -1), self.bl
        vb[:, :wf], vb[:, wf:wf + self.ways] = self.wld.reshape(T, -1), self.bld
        return dev(pb), dev(vb), ps, vs, gs

    def ref_primal(self, dtype=torch.float64):
        out = []
        for t in range(self.T):
            a = [torch.from_numpy(x[t]).to(dtype) for x in (self.f, self.wl, self.bl)]
            out.append(KR.head_fwd_bwd(*a, torch.from_numpy(self.y[t]).long()))
        return out


_PRIMAL_KEYS = ('loss', 'logits', 'prob', 'dl', 'dwl', 'dbl', 'df')
_PRIMAL_BARS = dict(loss=2e-6, logits=5e-6, prob=5e-6, dl=5e-6, dwl=5e-6, dbl=5e-6, df=5e-6)
_ABS_KEYS = ('loss', 'logits', 'prob', 'ld', 'pd', 'p')


def _err(key, got, want):
    return max_err(got, want) if key in _ABS_KEYS else rel_err(got, want)


def run_head_primal(lib, hc):
    T, n, feat, ways = hc.T, hc.n, hc.feat, hc.ways
    pb, _, ps, _, gs = hc.pack()
    fdv, yd = dev(hc.f), dev(hc.y, torch.int32)
    o = dict(loss=_nan(T), acc=_nan(T), logits=_nan(T, n, ways), prob=_nan(T, n, ways), dl=_nan(T, n, ways), g=_nan(T, gs), df=_nan(T, n, feat))
    wf = ways * feat
    rc = lib.mi_head_fwd_bwd(stream(), ptr(fdv), ptr(pb), _at(pb, wf), ps, ptr(yd), T, n, feat, ways, ptr(o['loss']), ptr(o['acc']),
                             ptr(o['logits']), ptr(o['prob']), ptr(o['dl']), ptr(o['g']), _at(o['g'], wf), gs, ptr(o['df']))
    torch.cuda.synchronize()
    o['dwl'], o['dbl'] = o['g'][:, :wf].reshape(T, ways, feat), o['g'][:, wf:wf + ways]
    return rc, o


def check_head_primal(name, hc, o, yard=None):
    """Kernel outputs against fp64.  yard: per-key fp32-reference error (only the cases the module docstring names pass one)."""
    ref = hc.ref_primal()
    errs = {k: 0.0 for k in _PRIMAL_KEYS}
    for t in range(hc.T):
        lr_, ar, lg, pr, dlr, dwr, dbr, dfr = ref[t]
        want = dict(loss=lr_, logits=lg, prob=pr, dl=dlr, dwl=dwr, dbl=dbr, df=dfr)
        for k in _PRIMAL_KEYS:
            errs[k] = max(errs[k], _err(k, _np(o[k][t]), want[k].numpy()))
        assert o['acc'][t].item() == ar.item(), (name, t)
    bars = dict(_PRIMAL_BARS)
    if yard is not None:
        report(f'head_primal_yardstick[{name}]', **{k: yard[k] for k in _PRIMAL_KEYS})
        bars = {k: max(bars[k], 4.0 * yard[k]) for k in bars}
    report(f'head_primal[{name}]', **errs)
    for k in _PRIMAL_KEYS:
        assert np.isfinite(errs[k]) and errs[k] < bars[k], (name, k, errs[k], bars[k])
    return errs


def primal_yardstick(hc):
    """Error of the fp64 reference code run in fp32 on the same inputs, against fp64."""
    r64, r32 = hc.ref_primal(), hc.ref_primal(torch.float32)
    yard = {k: 0.0 for k in _PRIMAL_KEYS}
    for a, b in zip(r64, r32):
        w64 = dict(loss=a[0], logits=a[2], prob=a[3], dl=a[4], dwl=a[5], dbl=a[6], df=a[7])
        w32 = dict(loss=b[0], logits=b[2], prob=b[3], dl=b[4], dwl=b[5], dbl=b[6], df=b[7])
        for k in _PRIMAL_KEYS:
            yard[k] = max(yard[k], _err(k, w32[k].numpy(), w64[k].numpy()))
    return yard


def saved_primal(hc):
    """prob, dl of the primal pass as the tangent kernels receive them: the fp64 reference's, rounded to fp32."""
    ref = hc.ref_primal()
    return (np.stack([r[3].numpy() for r in ref]).astype(np.float32), np.stack([r[4].numpy() for r in ref]).astype(np.float32))


def run_head_tangent(lib, hc, prob, dl, mode):
    """mode 'fd': with feature tangents; 'nofd': fd == NULL; 'fixed': fixed_dl = 1 with ld_out (dl is then any given cotangent)."""
    T, n, feat, ways = hc.T, hc.n, hc.feat, hc.ways
    pb, vb, ps, vs, gs = hc.pack()
    wf = ways * feat
    fdv, fdd, pd_, dld = dev(hc.f), dev(hc.fd), dev(prob), dev(dl)
    o = dict(rdl=_nan(T, n, ways), ld=_nan(T, n, ways), g=_nan(T, gs), df=_nan(T, n, feat))
    rc = lib.mi_head_tangent(stream(), ptr(fdv), ptr(fdd) if mode != 'nofd' else None, ptr(pb), _at(pb, wf), ps, ptr(vb), _at(vb, wf), vs,
                             ptr(pd_) if mode != 'fixed' else None, ptr(dld), ptr(o['rdl']), ptr(o['ld']), 1 if mode == 'fixed' else 0,
                             T, n, feat, ways, ptr(o['g']), _at(o['g'], wf), gs, ptr(o['df']))
    torch.cuda.synchronize()
    o['dwl'], o['dbl'] = o['g'][:, :wf].reshape(T, ways, feat), o['g'][:, wf:wf + ways]
    return rc, o


def ref_head_tangent(hc, prob, dl, mode, dtype=torch.float64):
    out = []
    for t in range(hc.T):
        f, fd, wl, bl, wld, bld, pr, d = [torch.from_numpy(x[t]).to(dtype) for x in (hc.f, hc.fd, hc.wl, hc.bl, hc.wld, hc.bld, prob, dl)]
        if mode == 'fixed':
            ld, rdwl, rdbl, rdf = KR.head_tangent_fixed_dl(f, fd, wl, wld, bld, d)
            out.append(dict(ld=ld, rdl=torch.zeros_like(ld), dwl=rdwl, dbl=rdbl, df=rdf))
            continue
        fdt = fd if mode == 'fd' else torch.zeros_like(fd)
        ld = KR.head_logit_tangent(f, fdt, wl, wld, bld)
        rdwl, rdbl, rdf = KR.head_tangent(f, fdt, wl, bl, wld, bld, pr, d)
        out.append(dict(ld=ld, rdl=KR.head_rdl(pr, ld), dwl=rdwl, dbl=rdbl, df=rdf))
    return out


_TAN_KEYS = ('ld', 'rdl', 'dwl', 'dbl', 'df')
_TAN_BARS = dict(ld=1e-5, rdl=5e-6, dwl=5e-6, dbl=5e-6, df=5e-6)


def check_head_tangent(name, hc, prob, dl, mode, o, use_yard=False):
    ref = ref_head_tangent(hc, prob, dl, mode)
    errs = {k: 0.0 for k in _TAN_KEYS}
    for t in range(hc.T):
        for k in _TAN_KEYS:
            errs[k] = max(errs[k], _err(k, _np(o[k][t]), ref[t][k].numpy()))
    bars = dict(_TAN_BARS)
    if use_yard:
        r32 = ref_head_tangent(hc, prob, dl, mode, torch.float32)
        yard = {k: max(_err(k, r32[t][k].numpy(), ref[t][k].numpy()) for t in range(hc.T)) for k in _TAN_KEYS}
        report(f'head_tangent_yardstick[{name},{mode}]', **yard)
        bars = {k: max(bars[k], 4.0 * yard[k]) for k in bars}
    report(f'head_tangent[{name},{mode}]', **errs)
    for k in _TAN_KEYS:
        assert np.isfinite(errs[k]) and errs[k] < bars[k], (name, mode, k, errs[k], bars[k])
    if mode == 'fixed':                                       # a given cotangent has no tangent of its own: exact zeros
        assert torch.count_nonzero(o['rdl']) == 0 and torch.count_nonzero(o['dbl']) == 0
    return errs


def run_head_grads(lib, hc, dl):
    T, n, feat, ways = hc.T, hc.n, hc.feat, hc.ways
    pb, _, ps, _, gs = hc.pack()
    wf = ways * feat
    fdv, dld = dev(hc.f), dev(dl)
    o = dict(g=_nan(T, gs), df=_nan(T, n, feat))
    rc = lib.mi_head_grads(stream(), ptr(fdv), ptr(pb), ps, ptr(dld), T, n, feat, ways, ptr(o['g']), _at(o['g'], wf), gs, ptr(o['df']))
    torch.cuda.synchronize()
    o['dwl'], o['dbl'] = o['g'][:, :wf].reshape(T, ways, feat), o['g'][:, wf:wf + ways]
    return rc, o


# (name, ways, n, feat, through mi_head_fwd_bwd as well)
HEAD_CASES = [
    ('one_class', 1, 3, 64, True),
    ('min_vector', 2, 1, 4, True),
    ('last_vector_width_two_rounds', 8, 33, 800, True),
    ('first_serial_width', 9, 5, 64, True),
    ('half_wave_of_classes', 33, 7, 68, True),
    ('header_cap', 64, 64, 64, True),
    ('scalar_partial_chunk_100', 5, 6, 100, False),
    ('scalar_partial_chunk_30', 5, 6, 30, False),
    ('guard_512_25_chunks', 5, 25, 1600, True),
]


@pytest.mark.parametrize('name,ways,n,feat,primal', HEAD_CASES)
def test_head_at_every_path(lib, name, ways, n, feat, primal):
    """Primal (mi_head_fwd_bwd, or mi_head_grads alone where the case says so) and the tangent three ways, T = 3 tasks of which task 1 is off the
    16-byte boundary."""
    hc = HeadCase(3, n, feat, ways)
    assert {0, ways - 1} <= set(hc.y.ravel().tolist())
    prob, dl = saved_primal(hc)
    if primal:
        rc, o = run_head_primal(lib, hc)
        _lib.check(rc)
        check_head_primal(name, hc, o)
        if ways == 1:                                         # one class: softmax is exactly 1, the loss exactly 0
            assert torch.all(o['loss'] == 0) and torch.all(o['dl'] == 0) and torch.all(o['prob'] == 1) and torch.all(o['acc'] == 1)
    rc, o = run_head_grads(lib, hc, dl)
    _lib.check(rc)
    dl64 = _t64(dl)
    e = dict(dwl=0.0, dbl=0.0, df=0.0)
    for t in range(hc.T):
        f, wl = _t64(hc.f[t]), _t64(hc.wl[t])
        want = dict(dwl=dl64[t].t() @ f, dbl=dl64[t].sum(dim=0), df=dl64[t] @ wl)
        for k in e:
            e[k] = max(e[k], rel_err(_np(o[k][t]), want[k].numpy()))
    report(f'head_grads[{name}]', **e)
    assert all(np.isfinite(v) and v < 5e-6 for v in e.values()), e
    for mode in ('fd', 'nofd', 'fixed'):
        rc, o = run_head_tangent(lib, hc, prob, dl, mode)
        _lib.check(rc)
        check_head_tangent(name, hc, prob, dl, mode, o)


def test_head_ties_take_the_first_maximal_class(lib):
    """Two identical weight rows with equal biases give exactly equal logits; lifted above the rest they tie for the maximum in every row: a row
    labelled with the first of them is a hit, one labelled with the second is not (torch.argmax's rule)."""
    hc = HeadCase(3, 6, 64, 5, seed=50)
    first, second = 1, 3
    hc.wl[:, second] = hc.wl[:, first]
    hc.bl[:, first] = hc.bl[:, second] = 2.5              # (no higher: with both at softmax 1/2, dl[first] + dl[second] cancels and df loses its digits)
    hc.y = np.array([[first, second, first, second, second, 0], [second] * 6, [first] * 6], np.int32)
    rc, o = run_head_primal(lib, hc)
    _lib.check(rc)
    lg = _np(o['logits'])
    assert np.array_equal(lg[:, :, first], lg[:, :, second]) and np.all(lg.argmax(axis=2) == first)
    assert [float(a) for a in _np(o['acc'])] == [np.float32(2) / np.float32(6), 0.0, 1.0]
    check_head_primal('ties', hc, o)


@pytest.mark.parametrize('feat', [64, 800])
def test_head_large_logits_stay_finite(lib, feat):
    """Weights scaled until the logits reach +-90: exp() of an unshifted logit would overflow, the shifted softmax does not."""
    hc = HeadCase(3, 6, feat, 5, seed=60, wscale=1.0)
    lg = np.einsum('tnf,twf->tnw', hc.f.astype(np.float64), hc.wl.astype(np.float64))
    hc.wl = (hc.wl * (90.0 / np.abs(lg).max())).astype(np.float32)
    hc.bl[:] = 0.0
    rc, o = run_head_primal(lib, hc)
    _lib.check(rc)
    assert 85.0 < float(o['logits'].abs().max()) < 95.0
    for k in ('loss', 'prob', 'dl', 'dwl', 'dbl', 'df'):
        assert bool(torch.isfinite(o[k]).all()), k
    check_head_primal(f'large_logits_{feat}', hc, o, yard=primal_yardstick(hc))


@pytest.mark.parametrize('ways', [64, 8])
def test_head_at_the_largest_n_times_ways_that_fits_lds(lib, ways):
    """The tangent gradient launch keeps R{dl} and dl of a task in LDS: n * ways <= 19712 fills the CU's 160 KiB exactly (64 ways) or to within
    one row (8 ways).  The primal pass runs at the same n (its own limit is twice as far)."""
    n = _largest_n(ways, 1)
    assert n == {64: 308, 8: 2464}[ways] and _head_lds(n, ways, 1) <= HEAD_LDS_LIMIT < _head_lds(n + 1, ways, 1)
    hc = HeadCase(2, n, 8, ways, seed=70)
    rc, o = run_head_primal(lib, hc)
    _lib.check(rc)
    check_head_primal(f'lds_limit_{ways}', hc, o, yard=primal_yardstick(hc))
    prob, dl = saved_primal(hc)
    for mode in ('fd', 'fixed'):
        rc, o = run_head_tangent(lib, hc, prob, dl, mode)
        _lib.check(rc)
        check_head_tangent(f'lds_limit_{ways}', hc, prob, dl, mode, o, use_yard=True)


@pytest.mark.parametrize('ways', [64, 8])
def test_head_refuses_the_first_n_that_does_not_fit(lib, ways):
    """One row more than fits: MI_ERR_ARG naming n, ways and the byte counts, nothing launched (every output still NaN) -- tangent at its limit,
    primal at its own."""
    n = _largest_n(ways, 1) + 1
    hc = HeadCase(1, n, 8, ways, seed=71)
    prob, dl = np.zeros((1, n, ways), np.float32), np.zeros((1, n, ways), np.float32)
    rc, o = run_head_tangent(lib, hc, prob, dl, 'fd')
    assert rc == -1
    msg = lib.mi_last_error(None).decode()
    assert f'n = {n}' in msg and f'ways = {ways}' in msg and str(_head_lds(n, ways, 1)) in msg and str(HEAD_LDS_LIMIT) in msg, msg
    assert all(_all_nan(o[k]) for k in ('rdl', 'ld', 'g', 'df'))
    n = _largest_n(ways, 0) + 1
    assert n == {64: 617, 8: 4929}[ways]
    hc = HeadCase(1, n, 8, ways, seed=72)
    rc, o = run_head_primal(lib, hc)
    assert rc == -1
    msg = lib.mi_last_error(None).decode()
    assert f'n = {n}' in msg and f'ways = {ways}' in msg and str(_head_lds(n, ways, 0)) in msg, msg
    assert all(_all_nan(o[k]) for k in ('loss', 'acc', 'logits', 'prob', 'dl', 'g', 'df'))
    rc, o = run_head_grads(lib, hc, np.zeros((1, n, ways), np.float32))
    assert rc == -1 and _all_nan(o['g']) and _all_nan(o['df'])


# ------------------------------------------------------------------------------------------------------------ spatial mean
@pytest.mark.parametrize('rows,hw,c', [(3, 1, 64), (5, 4, 64), (7, 9, 32)])
def test_spatial_mean_fwd_bwd(lib, rows, hw, c):
    p, df = _rand(80, (rows, hw, c), -1.0, 2.0), _rand(81, (rows, c))
    pdv, dfd = dev(p), dev(df)
    f, dp = _nan(rows, c), _nan(rows, hw, c)
    _lib.check(lib.mi_spatial_mean(stream(), ptr(pdv), ptr(f), rows, hw, c))
    _lib.check(lib.mi_spatial_mean_bwd(stream(), ptr(dfd), ptr(dp), rows, hw, c))
    torch.cuda.synchronize()
    e = dict(f=rel_err(_np(f), KR.spatial_mean(_t64(p)).numpy()), dp=rel_err(_np(dp), KR.spatial_mean_bwd(_t64(df), hw).numpy()))
    report(f'spatial_mean[{rows},{hw},{c}]', **e)
    assert e['f'] < 1e-6 and e['dp'] < 1e-6
    assert np.array_equal(_np(dp), np.broadcast_to((df / np.float32(hw))[:, None, :], (rows, hw, c)))   # one fp32 division, nothing else


# ------------------------------------------------------------------------------------------------------------ the one-launch tail
class TailCase:
    """Inputs of one tail case.  Per-task vectors: theta = [gamma | beta | (shift) | wl | bl | pad], the direction likewise, the gradients
    [dgamma | dbeta | dwl | dbl | pad]; strides are multiples of 4 floats (the BatchNorm vectors are read 16 bytes at a time).  wl_shift = 1
    puts the head weights off the 16-byte boundary (the tail then copies them to LDS one float at a time)."""

    def __init__(self, T, n, ho, wo, c, pool, ways, seed=100, wl_shift=0):
        self.T, self.n, self.ho, self.wo, self.c, self.pool, self.ways, self.shift = T, n, ho, wo, c, pool, ways, wl_shift
        self.hp, self.wp = (ho // 2, wo // 2) if pool else (ho, wo)
        self.feat = feat = self.hp * self.wp * c
        self.z = _rand(seed, (T, n, ho, wo, c), -2.0, 3.0)
        self.zd = _rand(seed + 1, (T, n, ho, wo, c), -1.0, 1.0)
        self.gamma, self.beta = _rand(seed + 2, (T, c), 0.1, 1.0), _rand(seed + 3, (T, c), -0.3, 0.3)
        self.gammad, self.betad = _rand(seed + 4, (T, c)), _rand(seed + 5, (T, c))
        self.wl, self.bl = _rand(seed + 6, (T, ways, feat), -0.1, 0.1), _rand(seed + 7, (T, ways), -0.1, 0.1)
        self.wld, self.bld = _rand(seed + 8, (T, ways, feat), -0.05, 0.05), _rand(seed + 9, (T, ways), -0.1, 0.1)
        self.y = _labels(T, n, ways)
        zt, zdt = _t64(self.z), _t64(self.zd)
        mu = zt.mean(dim=(1, 2, 3))
        rstd = 1.0 / torch.sqrt(zt.var(dim=(1, 2, 3), unbiased=False) + KR.EPS)
        self.mu, self.rstd = mu.float().numpy(), rstd.float().numpy()
        zh = (zt - _t64(self.mu)[:, None, None, None]) * _t64(self.rstd)[:, None, None, None]
        self.m1 = zdt.mean(dim=(1, 2, 3)).float().numpy()
        self.m2 = (zh * zdt).mean(dim=(1, 2, 3)).float().numpy()
        self.o_gamma, self.o_beta, self.o_wl = 0, c, 2 * c + wl_shift
        self.o_bl = self.o_wl + ways * feat
        self.stride = (self.o_bl + ways + 3) // 4 * 4 + 4
        self.g_wl, self.g_bl = 2 * c, 2 * c + ways * feat
        self.gstride = (self.g_bl + ways + 3) // 4 * 4 + 8

    def task(self, t):
        """The same case reduced to task t alone."""
        import copy
        s = copy.copy(self)
        s.T = 1
        for k in ('z', 'zd', 'gamma', 'beta', 'gammad', 'betad', 'wl', 'bl', 'wld', 'bld', 'y', 'mu', 'rstd', 'm1', 'm2'):
            setattr(s, k, getattr(self, k)[t:t + 1])
        return s

    def theta(self, direction=False):
        b = np.zeros((self.T, self.stride), np.float32)
        parts = (self.gammad, self.betad, self.wld, self.bld) if direction else (self.gamma, self.beta, self.wl, self.bl)
        for off, a in zip((self.o_gamma, self.o_beta, self.o_wl, self.o_bl), parts):
            b[:, off:off + a[0].size] = a.reshape(self.T, -1)
        return dev(b)

    def supported(self, lib, n=None):
        return lib.mi_tail_supported(self.n if n is None else n, self.ho, self.wo, self.c, self.pool, self.feat, self.ways)


def tail_scratch(lib, tc):
    sb = lib.mi_tail_scratch_bytes(tc.T, tc.n, tc.ho, tc.wo, tc.c, tc.pool, tc.ways)
    assert sb > 0
    return torch.zeros(sb, dtype=torch.uint8, device='cuda'), sb       # zeroed once: the arrival counters are the caller's to clear


def run_tail(lib, tc, tangent=0, saved=None, with_grad=1, bwd_tasks=None, scratch=None):
    """One launch of the tail.  saved (tangent): the primal run's outputs (p, prob, dl, df).  -> (rc, outputs)."""
    T, n, c, ways, feat = tc.T, tc.n, tc.c, tc.ways, tc.feat
    th, vd = tc.theta(), tc.theta(True)
    keep = [th, vd, dev(tc.z), dev(tc.zd), dev(tc.mu), dev(tc.rstd), dev(tc.m1), dev(tc.m2), dev(tc.y, torch.int32)]
    zdv, zdd, mud, rd, m1d, m2d, yd = keep[2:]
    o = dict(pooled=_nan(T, n, tc.hp, tc.wp, c), loss=_nan(T), acc=_nan(T), logits=_nan(T, n, ways), g=_nan(T, tc.gstride), df=_nan(T, n, feat))
    if tangent:
        o['prob'], o['dl'] = saved['prob'].clone(), saved['dl'].clone()
        fsv, dpsv = saved['pooled'].clone(), saved['df'].clone()
    else:
        o['prob'], o['dl'] = _nan(T, n, ways), _nan(T, n, ways)
        fsv = dpsv = None
    a = _lib.MiTailArgs(z=zdv.data_ptr(), zd=zdd.data_ptr(), mu=mud.data_ptr(), rstd=rd.data_ptr(), m1=m1d.data_ptr(), m2=m2d.data_ptr(),
                        gamma=th.data_ptr() + 4 * tc.o_gamma, beta=th.data_ptr() + 4 * tc.o_beta, wl=th.data_ptr() + 4 * tc.o_wl,
                        bl=th.data_ptr() + 4 * tc.o_bl, pstride=tc.stride,
                        gammad=vd.data_ptr() + 4 * tc.o_gamma, betad=vd.data_ptr() + 4 * tc.o_beta, wld=vd.data_ptr() + 4 * tc.o_wl,
                        bld=vd.data_ptr() + 4 * tc.o_bl, vstride=tc.stride, y=yd.data_ptr(),
                        f=fsv.data_ptr() if tangent else None, dp=dpsv.data_ptr() if tangent else None,
                        prob=o['prob'].data_ptr(), dl=o['dl'].data_ptr(), pooled=o['pooled'].data_ptr(), loss=o['loss'].data_ptr(),
                        acc=o['acc'].data_ptr(), logits=o['logits'].data_ptr(), dwl=o['g'].data_ptr() + 4 * tc.g_wl,
                        dbl=o['g'].data_ptr() + 4 * tc.g_bl, sum0=o['g'].data_ptr(), sum1=o['g'].data_ptr() + 4 * c, gstride=tc.gstride,
                        df=o['df'].data_ptr(), tasks=T, n=n, ho=tc.ho, wo=tc.wo, c=c, pool=tc.pool, ways=ways, with_grad=with_grad,
                        bwd_tasks=T if bwd_tasks is None else bwd_tasks)
    if scratch is None:
        scratch = tail_scratch(lib, tc)
    rc = lib.mi_tail_run(stream(), C.byref(a), tangent, ptr(scratch[0]), scratch[1])
    torch.cuda.synchronize()
    del keep
    o['dgamma'], o['dbeta'] = o['g'][:, :c], o['g'][:, c:2 * c]
    o['dwl'], o['dbl'] = o['g'][:, tc.g_wl:tc.g_wl + ways * feat].reshape(T, ways, feat), o['g'][:, tc.g_bl:tc.g_bl + ways]
    return rc, o


def run_separate_primal(lib, tc):
    """mi_bn_relu_pool, then mi_head_fwd_bwd on its output."""
    T, n, c, ways, feat = tc.T, tc.n, tc.c, tc.ways, tc.feat
    th = tc.theta()
    zdv, mud, rd, yd = dev(tc.z), dev(tc.mu), dev(tc.rstd), dev(tc.y, torch.int32)
    o = dict(pooled=_nan(T, n, tc.hp, tc.wp, c), loss=_nan(T), acc=_nan(T), logits=_nan(T, n, ways), prob=_nan(T, n, ways), dl=_nan(T, n, ways),
             g=_nan(T, tc.gstride), df=_nan(T, n, feat))
    _lib.check(lib.mi_bn_relu_pool(stream(), ptr(zdv), ptr(mud), ptr(rd), _at(th, tc.o_gamma), _at(th, tc.o_beta), tc.stride, T, n, tc.ho, tc.wo,
                                   c, tc.pool, ptr(o['pooled'])))
    _lib.check(lib.mi_head_fwd_bwd(stream(), ptr(o['pooled']), _at(th, tc.o_wl), _at(th, tc.o_bl), tc.stride, ptr(yd), T, n, feat, ways,
                                   ptr(o['loss']), ptr(o['acc']), ptr(o['logits']), ptr(o['prob']), ptr(o['dl']), _at(o['g'], tc.g_wl),
                                   _at(o['g'], tc.g_bl), tc.gstride, ptr(o['df'])))
    torch.cuda.synchronize()
    o['dwl'], o['dbl'] = o['g'][:, tc.g_wl:tc.g_wl + ways * feat].reshape(T, ways, feat), o['g'][:, tc.g_bl:tc.g_bl + ways]
    return o


def run_separate_tangent(lib, tc, saved):
    """mi_bn_tangent_fwd, then mi_head_tangent on its output and the primal pass's stored features / softmax / dlogits."""
    T, n, c, ways, feat = tc.T, tc.n, tc.c, tc.ways, tc.feat
    th, vd = tc.theta(), tc.theta(True)
    zdv, zdd, mud, rd, m1d, m2d = dev(tc.z), dev(tc.zd), dev(tc.mu), dev(tc.rstd), dev(tc.m1), dev(tc.m2)
    a = _lib.MiBnTangentArgs(z=zdv.data_ptr(), zd=zdd.data_ptr(), mu=mud.data_ptr(), rstd=rd.data_ptr(), m1=m1d.data_ptr(), m2=m2d.data_ptr(),
                             gamma=th.data_ptr() + 4 * tc.o_gamma, beta=th.data_ptr() + 4 * tc.o_beta, pstride=tc.stride,
                             gammad=vd.data_ptr() + 4 * tc.o_gamma, betad=vd.data_ptr() + 4 * tc.o_beta, vstride=tc.stride,
                             tasks=T, n=n, ho=tc.ho, wo=tc.wo, c=c, pool=tc.pool)
    o = dict(pooled=_nan(T, n, tc.hp, tc.wp, c), rdl=_nan(T, n, ways), g=_nan(T, tc.gstride), df=_nan(T, n, feat))
    _lib.check(lib.mi_bn_tangent_fwd(stream(), C.byref(a), ptr(o['pooled'])))
    _lib.check(lib.mi_head_tangent(stream(), ptr(saved['pooled']), ptr(o['pooled']), _at(th, tc.o_wl), _at(th, tc.o_bl), tc.stride,
                                   _at(vd, tc.o_wl), _at(vd, tc.o_bl), tc.stride, ptr(saved['prob']), ptr(saved['dl']), ptr(o['rdl']), None, 0,
                                   T, n, feat, ways, _at(o['g'], tc.g_wl), _at(o['g'], tc.g_bl), tc.gstride, ptr(o['df'])))
    torch.cuda.synchronize()
    o['dwl'], o['dbl'] = o['g'][:, tc.g_wl:tc.g_wl + ways * feat].reshape(T, ways, feat), o['g'][:, tc.g_bl:tc.g_bl + ways]
    return o


_TAIL_BARS = dict(p=5e-6, loss=2e-6, logits=5e-6, prob=5e-6, dl=5e-6, dwl=5e-6, dbl=5e-6, df=5e-6, dgamma=5e-6, dbeta=5e-6)
_TAIL_TAN_BARS = dict(pd=1e-5, rdwl=5e-6, rdbl=5e-6, rdf=5e-6, rdgamma=5e-6, rdbeta=5e-6)


def check_tail_primal(name, tc, o):
    errs = {k: 0.0 for k in _TAIL_BARS}
    got = dict(o, p=o['pooled'])
    for t in range(tc.T):
        r = KR.tail_ref(_t64(tc.z[t]), _t64(tc.mu[t]), _t64(tc.rstd[t]), _t64(tc.gamma[t]), _t64(tc.beta[t]), _t64(tc.wl[t]), _t64(tc.bl[t]),
                        torch.from_numpy(tc.y[t]).long(), bool(tc.pool))
        for k in errs:
            errs[k] = max(errs[k], _err(k, _np(got[k][t]).reshape(r[k].shape), r[k].numpy()))
        assert o['acc'][t].item() == r['acc'].item(), (name, t)
    report(f'tail_primal[{name}]', **errs)
    for k, bar in _TAIL_BARS.items():
        assert np.isfinite(errs[k]) and errs[k] < bar, (name, k, errs[k], bar)


def check_tail_tangent(name, tc, saved, o):
    errs = {k: 0.0 for k in _TAIL_TAN_BARS}
    got = dict(pd=o['pooled'], rdwl=o['dwl'], rdbl=o['dbl'], rdf=o['df'], rdgamma=o['dgamma'], rdbeta=o['dbeta'])
    for t in range(tc.T):
        r = KR.tail_tangent_ref(_t64(tc.z[t]), _t64(tc.zd[t]), _t64(tc.mu[t]), _t64(tc.rstd[t]), _t64(tc.m1[t]), _t64(tc.m2[t]),
                                _t64(tc.gamma[t]), _t64(tc.beta[t]), _t64(tc.gammad[t]), _t64(tc.betad[t]), _t64(tc.wl[t]), _t64(tc.bl[t]),
                                _t64(tc.wld[t]), _t64(tc.bld[t]), saved['pooled'][t].double().cpu().reshape(tc.n, -1),
                                saved['prob'][t].double().cpu(), saved['dl'][t].double().cpu(), saved['df'][t].double().cpu(), bool(tc.pool))
        for k in errs:
            errs[k] = max(errs[k], (max_err if k == 'pd' else rel_err)(_np(got[k][t]).reshape(r[k].shape), r[k].numpy()))
    report(f'tail_tangent[{name}]', **errs)
    for k, bar in _TAIL_TAN_BARS.items():
        assert np.isfinite(errs[k]) and errs[k] < bar, (name, k, errs[k], bar)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b, keys, what):
    for k in keys:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k)


_BITS_PRIMAL = ('pooled', 'logits', 'prob', 'dl', 'loss', 'acc', 'dwl', 'dbl', 'df')
_BITS_TANGENT = ('pooled', 'dwl', 'dbl', 'df')

# (name, T, n, ho, wo, c, pool, ways, the first refused n or None)
TAIL_CASES = [
    ('min_last_block_items_cap', 2, 40, 10, 10, 32, 1, 8, 41),
    ('omni_last_block_items_cap', 2, 128, 2, 2, 64, 0, 5, 129),
    ('omni_last_block_row_scalar_cap', 2, 102, 2, 2, 64, 0, 8, 103),
    ('odd_map', 3, 5, 5, 5, 32, 1, 5, None),
    ('rect_odd_map', 3, 6, 3, 5, 64, 1, 3, None),
    ('one_row', 3, 1, 4, 4, 32, 1, 1, None),
    ('two_rows', 3, 2, 4, 4, 32, 1, 1, None),
    ('three_rows', 3, 3, 4, 4, 32, 1, 1, None),
    ('c4', 3, 5, 2, 2, 4, 0, 2, None),
    ('c256', 2, 5, 2, 2, 256, 0, 2, None),
    ('lds_cap', 2, 20, 3, 3, 128, 0, 8, 21),
]


@pytest.mark.parametrize('name,T,n,ho,wo,c,pool,ways,refused', TAIL_CASES)
def test_tail_against_fp64_and_the_separate_launches(lib, name, T, n, ho, wo, c, pool, ways, refused):
    tc = TailCase(T, n, ho, wo, c, pool, ways)
    assert tc.supported(lib) == 1
    if name == 'odd_map':                                     # 9 windows for 4 pooled outputs: the last row and column feed nothing
        assert ((ho + 1) // 2) * ((wo + 1) // 2) == 9 and tc.hp * tc.wp == 4
    if name == 'lds_cap':                                     # the 150 KiB bound alone decides: the other limits hold at n + 1 as well
        rl = (refused + 3) // 4
        assert lib.mi_tail_lds_bytes(n, tc.feat, ways, 1) <= 150 * 1024 < lib.mi_tail_lds_bytes(refused, tc.feat, ways, 1)
        assert rl * ho * wo * (c // 4) <= 4 * 512 and refused * (ways + 2) <= 2 * 512
    rc, o = run_tail(lib, tc)
    _lib.check(rc)
    check_tail_primal(name, tc, o)
    _same_bits(o, run_separate_primal(lib, tc), _BITS_PRIMAL, f'{name}: tail vs separate launches')
    rc, ot = run_tail(lib, tc, tangent=1, saved=o)
    _lib.check(rc)
    check_tail_tangent(name, tc, o, ot)
    _same_bits(ot, run_separate_tangent(lib, tc, o), _BITS_TANGENT, f'{name}: tangent tail vs separate launches')
    if refused is not None:
        big = TailCase(1, refused, ho, wo, c, pool, ways)
        assert big.supported(lib) == 0
        rc, ob = run_tail(lib, big)
        assert rc == -1 and 'tail' in lib.mi_last_error(None).decode()
        assert all(_all_nan(ob[k]) for k in ('pooled', 'loss', 'acc', 'logits', 'prob', 'dl', 'g', 'df'))


@pytest.mark.parametrize('name,n,ho,wo,c,pool,ways', [('c12', 5, 2, 2, 12, 0, 2), ('ways9', 5, 2, 2, 32, 0, 9), ('c260', 5, 2, 2, 260, 0, 2),
                                                      ('c6', 5, 2, 2, 6, 0, 2)])
def test_tail_refuses_what_its_kernels_do_not_take(lib, name, n, ho, wo, c, pool, ways):
    """512 threads do not divide into c / 4 = 3 channel quads; more than 8 classes; more than 256 channels; c not a multiple of 4."""
    feat = ho * wo * c
    assert lib.mi_tail_supported(n, ho, wo, c, pool, feat, ways) == 0
    if c % 4 == 0:
        tc = TailCase(1, n, ho, wo, c, pool, ways)
        rc, o = run_tail(lib, tc)
        assert rc == -1 and all(_all_nan(o[k]) for k in ('pooled', 'loss', 'g', 'df'))


def test_tail_supported_counts_the_partial_windows_of_an_odd_map(lib):
    """A pooled odd map has ceil(h/2) * ceil(w/2) windows to visit (the partial ones are visited and dropped) but floor * floor outputs: the items
    limit counts the former.  5 x 5 x 32 pooled: 9 windows x 8 quads = 72 items per row, 2048 / 72 = 28 rows per group -> n <= 112, where counting
    pooled outputs only (4 x 8 = 32 per row) would let n = 113 .. 256 through with items the kernel never visits."""
    feat = 2 * 2 * 32
    assert lib.mi_tail_supported(112, 5, 5, 32, 1, feat, 1) == 1
    assert lib.mi_tail_supported(113, 5, 5, 32, 1, feat, 1) == 0
    assert lib.mi_tail_supported(112, 5, 5, 32, 1, feat + 32, 1) == 0            # feat must be the pooled map's


def test_tail_at_the_window_count_limit_of_an_odd_map(lib):
    """n = 112 on the pooled 5 x 5 map: every thread holds its four items, a quarter of them partial windows.  Against fp64."""
    tc = TailCase(1, 112, 5, 5, 32, 1, 1, seed=130)
    rc, o = run_tail(lib, tc)
    _lib.check(rc)
    check_tail_primal('odd_map_items_cap', tc, o)
    rc, ot = run_tail(lib, tc, tangent=1, saved=o)
    _lib.check(rc)
    check_tail_tangent('odd_map_items_cap', tc, o, ot)
    big = TailCase(1, 113, 5, 5, 32, 1, 1, seed=130)          # one row more: a 29th row per group, 2088 items for 2048 slots
    rc, ob = run_tail(lib, big)
    assert rc == -1 and all(_all_nan(ob[k]) for k in ('pooled', 'loss', 'g', 'df'))


def test_tail_with_head_weights_off_the_16_byte_boundary(lib):
    """The tail copies unaligned head weights to LDS with its scalar loop; fp64 only (the separate head kernel then takes its scalar dot path, whose
    summation order differs)."""
    tc = TailCase(2, 6, 5, 5, 32, 1, 5, seed=140, wl_shift=1)
    rc, o = run_tail(lib, tc)
    _lib.check(rc)
    check_tail_primal('wl_unaligned', tc, o)
    rc, ot = run_tail(lib, tc, tangent=1, saved=o)
    _lib.check(rc)
    check_tail_tangent('wl_unaligned', tc, o, ot)


def test_tail_ties_and_row_hits(lib):
    """Equal logits inside the tail: the first maximal class wins, as in the separate kernel."""
    tc = TailCase(2, 6, 4, 4, 32, 1, 5, seed=150)
    tc.wl[:, 3] = tc.wl[:, 1]
    tc.bl[:, 1] = tc.bl[:, 3] = 2.5                           # (as in the head's tie test)
    tc.y = np.array([[1, 3, 1, 3, 3, 0], [1] * 6], np.int32)
    rc, o = run_tail(lib, tc)
    _lib.check(rc)
    lg = _np(o['logits'])
    assert np.array_equal(lg[:, :, 1], lg[:, :, 3]) and np.all(lg.argmax(axis=2) == 1)
    assert [float(a) for a in _np(o['acc'])] == [np.float32(2) / np.float32(6), 1.0]
    check_tail_primal('ties', tc, o)


def test_tail_forward_only_and_validation_tasks(lib):
    """with_grad = 0: loss, accuracy and the forward tensors only.  bwd_tasks = 1 of 3: tasks 1 and 2 stop after the loss, task 0 is its T = 1 run."""
    tc = TailCase(3, 5, 5, 5, 32, 1, 5, seed=160)
    rc, full = run_tail(lib, tc)
    _lib.check(rc)
    rc, fwd = run_tail(lib, tc, with_grad=0)
    _lib.check(rc)
    _same_bits(fwd, full, ('pooled', 'logits', 'prob', 'dl', 'loss', 'acc'), 'forward only')
    assert _all_nan(fwd['g']) and _all_nan(fwd['df'])
    rc, part = run_tail(lib, tc, bwd_tasks=1)
    _lib.check(rc)
    _same_bits(part, full, ('pooled', 'logits', 'prob', 'dl', 'loss', 'acc'), 'validation tasks')
    assert _all_nan(part['g'][1:]) and _all_nan(part['df'][1:])
    rc, alone = run_tail(lib, tc.task(0))
    _lib.check(rc)
    for k in _BITS_PRIMAL + ('dgamma', 'dbeta'):
        assert torch.equal(_bits(part[k][0]), _bits(alone[k][0])), k


@pytest.mark.parametrize('tangent', [0, 1])
def test_tail_counters_and_batch_independence(lib, tangent):
    """Two launches on the same scratch without clearing the arrival counters in between: the same bits, counters back at zero.  Every task of a
    T = 3 call is the same bits as that task launched alone."""
    tc = TailCase(3, 6, 3, 5, 64, 1, 3, seed=170)
    rc, prim = run_tail(lib, tc)
    _lib.check(rc)
    saved = prim if tangent else None
    scratch = tail_scratch(lib, tc)
    rc, a = run_tail(lib, tc, tangent=tangent, saved=saved, scratch=scratch)
    _lib.check(rc)
    assert torch.count_nonzero(scratch[0][:4 * tc.T]) == 0
    rc, b = run_tail(lib, tc, tangent=tangent, saved=saved, scratch=scratch)
    _lib.check(rc)
    assert torch.count_nonzero(scratch[0][:4 * tc.T]) == 0
    keys = (_BITS_TANGENT if tangent else _BITS_PRIMAL) + ('dgamma', 'dbeta')
    _same_bits(a, b, keys, 'second launch on the same scratch')
    for t in range(tc.T):
        sv = {k: prim[k][t:t + 1].contiguous() for k in ('pooled', 'prob', 'dl', 'df')} if tangent else None
        rc, one = run_tail(lib, tc.task(t), tangent=tangent, saved=sv)
        _lib.check(rc)
        for k in keys:
            assert torch.equal(_bits(a[k][t]), _bits(one[k][0])), (t, k)
