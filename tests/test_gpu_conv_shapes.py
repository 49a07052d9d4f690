"""The hidden-block convolution and weight-gradient kernels at every boundary of their launchers (tests/conv_shape_cases.py; what the table
covers is proved on the CPU by tests/test_conv_plan_host.py): every case, under every operand form of conftest.CONV_FORMS, through
mi_conv3x3_bn_stats, mi_conv3x3_bwd, mi_conv3x3_tangent and mi_conv3x3_bwd2 against the fp64 restatement (oracle/kernels_ref.py) on the
same fp32 inputs, at the bars of tests/test_gpu_kernels.py and tests/test_gpu_tangent_kernels.py: z, dx, mu / std, rstd and the tangent
statistics 2e-6, dW 5e-6.  Outputs start as NaN, the gradient rows are longer than 9 ci co and their tails must stay NaN, every test
asserts through mi_debug_wgrad_plan / mi_debug_conv_plan that the launch took the plan the table names, and cases of many tasks (a few
distinct tasks, repeated) hold every task to the single-task launch."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import conv_shape_cases as CS
from conftest import CONV_FORMS, apply_conv_form
from exploring_meta_amd import _lib
from oracle import kernels_ref as KR
from gpu_utils import dev, ptr, stream, rel_err, max_err, report, rand32 as _rand, t64 as _t64

pytestmark = pytest.mark.gpu

ND = 4                                                       # distinct tasks of a many-task case (repeated: the kernels do not know)
NAMES = [c.name for c in CS.CASES]
HIDDEN = [c.name for c in CS.CASES if c.ci >= 32]


@pytest.fixture(scope='module', params=list(CONV_FORMS))
def lib(request):
    lb = _lib.load()
    restore = apply_conv_form(lb, request.param)
    yield lb, request.param
    restore()


@functools.lru_cache(maxsize=None)
def _inputs(name):
    """The seeded tensors of a case (min(T, ND) distinct tasks), shared by every test and every form; never modified."""
    c = CS.BY_NAME[name]
    nd = min(c.T, ND)
    ho, wo = CS.out_hw(c)
    d = dict(nd=nd, ho=ho, wo=wo,
             x0=_rand(50, (nd, c.n, c.h, c.w, c.ci), 0.0, 2.0), x1=_rand(51, (nd, c.n, c.h, c.w, c.ci)),
             w0=_rand(52, (nd, 9, c.ci, c.co), -0.3, 0.3), w1=_rand(53, (nd, 9, c.ci, c.co), -0.3, 0.3),
             z=_rand(54, (nd, c.n, ho, wo, c.co), -2.0, 3.0), dz0=_rand(65, (nd, c.n, ho, wo, c.co)), dz1=_rand(66, (nd, c.n, ho, wo, c.co)))
    zt = torch.from_numpy(d['z']).double()
    d['mu'] = zt.mean(dim=(1, 2, 3)).float()
    d['rstd'] = (1.0 / torch.sqrt(zt.var(dim=(1, 2, 3), unbiased=False) + 1e-5)).float()
    d['checked'] = sorted({t % nd for t in (range(c.T) if c.check is None else c.check)})
    return d


@functools.lru_cache(maxsize=None)
def _ref(name, k, what):
    """fp64 reference of distinct task k, computed once and shared (returned tensors are read only)."""
    c, d = CS.BY_NAME[name], _inputs(name)
    s = c.stride
    if what == 'z':
        return KR.conv3x3(_t64(d['x0'][k]), _t64(d['w0'][k]), s)
    if what == 'z1':
        return KR.conv3x3(_t64(d['x1'][k]), _t64(d['w1'][k]), s)
    if what == 'dw':
        return KR.conv3x3_wgrad(_t64(d['x0'][k]), _t64(d['dz0'][k]), s)
    if what == 'dw1':
        return KR.conv3x3_wgrad(_t64(d['x1'][k]), _t64(d['dz1'][k]), s)
    if what == 'dx':
        return KR.conv3x3_dgrad(_t64(d['dz0'][k]), _t64(d['w0'][k]), (c.h, c.w), s)
    if what == 'dx1':
        return KR.conv3x3_dgrad(_t64(d['dz1'][k]), _t64(d['w1'][k]), (c.h, c.w), s)
    raise KeyError(what)


def _rep(a, T):
    """Distinct tasks [nd, ...] on the device, repeated to T tasks."""
    t = dev(a)
    nd = t.shape[0]
    return t if nd == T else t.repeat((T + nd - 1) // nd, *([1] * (t.dim() - 1)))[:T].contiguous()


def _weights(d, T, names, pad):
    """Per-task parameter rows [w | w' | pad floats]: returns (device buffer [T, stride], offsets in floats, stride)."""
    parts = [d[k].reshape(d['nd'], -1) for k in names]
    stride = sum(p.shape[1] for p in parts) + pad
    buf = np.zeros((d['nd'], stride), np.float32)
    offs, o = [], 0
    for p in parts:
        buf[:, o:o + p.shape[1]] = p
        offs.append(o)
        o += p.shape[1]
    return _rep(buf, T), offs, stride


def _at(buf, off):
    return C.c_void_p(buf.data_ptr() + 4 * off)


def _scratch(lb, c):
    sb = lb.mi_kernel_scratch_bytes(c.T, c.n, c.h, c.w, c.co)
    return torch.empty(sb, dtype=torch.uint8, device='cuda'), sb


def _nan(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def _all_written(**outs):
    """Output buffers start as NaN: every element of every task must have been written (the weight-gradient rows up to 9 ci co)."""
    for k, t in outs.items():
        if t is not None:
            assert bool(torch.isfinite(t).all()), f'{k}: {int((~torch.isfinite(t)).sum())} element(s) unwritten or not finite'


def _worse(e, key, val):
    """e[key] = the larger of the two -- after asserting that val is a number (max(0.0, nan) is 0.0: a NaN must not get lost here)."""
    assert np.isfinite(val), (key, val)
    e[key] = max(e[key], float(val))


def _edge_err(got, ref):
    """Largest error of an element of the map's first / last row or column, over max |ref| ([n, h, w, c] tensors): the whole-tensor
    2-norm of rel_err dilutes one bad boundary element of a larger map.  Held to the same 2e-6 in the maximum norm: an output is a sum
    of K = 9 ci (two terms: 18 ci) fp32 products, whose accumulated rounding is about sqrt(K) 2^-24 <= 1.5e-6 of the rms of such a sum,
    and max |ref| is several times that rms."""
    g, r = np.asarray(got, np.float64), ref.numpy()
    m = np.zeros(r.shape[1:3], bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    return float(np.max(np.abs(g - r)[:, m])) / max(float(np.max(np.abs(r))), 1e-300)


def _assert_conv_plan(lb, form, c, nterms, epi, mode):
    p = CS.case_conv_plan(lb, c, nterms, epi, mode)
    assert p.kernel == CS.expected_conv_kernel(c, form, nterms, p), (c.name, form, p)
    assert p.stats64 == CS.expected_stats64(p, epi), (c.name, form, p)
    if c.name == 'c_tpw2_13x13':
        assert p.tiles_per_wave > 1 and (c.n * c.h * c.w) % p.tile_pix != 0, p
    if c.name == 'c_tpw6_20x20' and form == 'split_bf16':
        assert p.tiles_per_wave >= 6 and p.kernel == 's1_bf16_16x16' and (c.n * c.h * c.w) % p.tile_pix != 0, p
    return p


def _assert_single_task(lb, form, c, nterms, epi, mode, plan, one, many, k):
    """A task of the many-task launch against the same task launched alone: the same bits where both launches take the same kernel
    (per-tile arithmetic does not depend on the tile split); where the tile count moves the launch to the other split-bf16 kernel
    (conftest 'split_bf16': 16x16x32 MFMAs from six tiles per wave) the two agree to the bar each is held to against fp64."""
    alone = CS.conv_plan(lb, 1, c.n, c.h, c.w, c.ci, c.co, c.stride, nterms, epi, mode)
    if alone.kernel == plan.kernel:
        assert torch.equal(one, many), (c.name, k)
    else:
        assert (c.name, form) == ('c_tpw6_20x20', 'split_bf16'), (c.name, form, alone.kernel, plan.kernel)      # the only such case and form
        assert rel_err(one.cpu().numpy(), many.cpu().numpy()) < 2e-6, (c.name, k, alone.kernel, plan.kernel)


def _assert_wgrad_plan(lb, form, c, nterms):
    p = CS.case_wgrad_plan(lb, c, nterms)
    assert (p.family, p.size, p.exact) == c.wgrad[(CS.form_kind(form), nterms)], (c.name, form, p)
    return p


@pytest.mark.parametrize('name', NAMES)
def test_conv_bn_stats_shapes(lib, name):
    """z, mu and rstd of mi_conv3x3_bn_stats.  (r4n_1x1, four values per channel with |mean| = 30 std in the worst one, is the case
    that made the 16x16x32 kernel take its fp64-statistics instance for tasks of one tile: rstd 3.3e-6 before, csrc/conv_b16.h S64.)"""
    lb, form = lib
    c, d = CS.BY_NAME[name], _inputs(name)
    T, nd, ho, wo = c.T, d['nd'], d['ho'], d['wo']
    plan = _assert_conv_plan(lb, form, c, 1, CS.EPI_STATS, 0)
    xd = _rep(d['x0'], T)
    wbuf, (o0,), pstride = _weights(d, T, ['w0'], 17)
    scratch, sb = _scratch(lb, c)

    def run(x, w, tasks):
        z, mu, rstd = _nan(tasks, c.n, ho, wo, c.co), _nan(tasks, c.co), _nan(tasks, c.co)
        _lib.check(lb.mi_conv3x3_bn_stats(stream(), ptr(x), ptr(w), pstride, tasks, c.n, c.h, c.w, c.ci, c.co, c.stride, ptr(z), ptr(mu),
                                          ptr(rstd), ptr(scratch), sb))
        torch.cuda.synchronize()
        return z, mu, rstd

    z, mu, rstd = run(xd, wbuf, T)
    _all_written(z=z, mu=mu, rstd=rstd)
    e = dict(z=0.0, z_edge=0.0, mu=0.0, rstd=0.0)
    for k in d['checked']:
        zr = _ref(name, k, 'z')
        m, r = KR.bn_stats(zr)
        _worse(e, 'z', rel_err(z[k].cpu().numpy(), zr.numpy()))
        _worse(e, 'z_edge', _edge_err(z[k].cpu().numpy(), zr))
        _worse(e, 'mu', max_err(mu[k].cpu().numpy(), m.numpy()) / max(1e-30, float(zr.std())))
        _worse(e, 'rstd', rel_err(rstd[k].cpu().numpy(), r.numpy()))
    if T > nd:
        for t in range(nd, T):                               # the same task anywhere in the launch: the same bits
            assert torch.equal(z[t], z[t % nd]), t
            assert torch.allclose(mu[t], mu[t % nd], rtol=1e-6, atol=1e-7) and torch.allclose(rstd[t], rstd[t % nd], rtol=1e-6)
        for k in range(nd):                                  # ... and the bits of the single-task launch
            z1, m1_, r1_ = run(xd[k], wbuf[k], 1)
            _assert_single_task(lb, form, c, 1, CS.EPI_STATS, 0, plan, z1[0], z[k], k)
            assert torch.allclose(m1_[0], mu[k], rtol=1e-6, atol=1e-7) and torch.allclose(r1_[0], rstd[k], rtol=1e-6)
    report(f'conv_shapes_bn_stats[{name}|{form}]', kernel=plan.kernel, tiles_per_wave=plan.tiles_per_wave, **e)
    assert e['z'] < 2e-6 and e['z_edge'] < 2e-6 and e['mu'] < 2e-6 and e['rstd'] < 2e-6, e


@pytest.mark.parametrize('name', NAMES)
def test_conv_bwd_shapes(lib, name):
    lb, form = lib
    c, d = CS.BY_NAME[name], _inputs(name)
    T, nd, ho, wo = c.T, d['nd'], d['ho'], d['wo']
    nw = 9 * c.ci * c.co
    wplan = _assert_wgrad_plan(lb, form, c, 1)
    need_dx = c.ci >= 32
    dplan = _assert_conv_plan(lb, form, c, 1, CS.EPI_NONE, 1) if need_dx else None
    xd, dzd = _rep(d['x0'], T), _rep(d['dz0'], T)
    wbuf, (o0,), pstride = _weights(d, T, ['w0'], 3)
    gstride = nw + 3
    scratch, sb = _scratch(lb, c)

    def run(x, dz, w, tasks):
        dx = _nan(tasks, c.n, c.h, c.w, c.ci) if need_dx else None
        dw = _nan(tasks, gstride)
        _lib.check(lb.mi_conv3x3_bwd(stream(), ptr(x), ptr(dz), ptr(w), pstride, tasks, c.n, c.h, c.w, c.ci, c.co, c.stride, ptr(dx), ptr(dw),
                                     gstride, ptr(scratch), sb))
        torch.cuda.synchronize()
        return dx, dw

    dx, dw = run(xd, dzd, wbuf, T)
    assert bool(torch.isnan(dw[:, nw:]).all()), 'the weight gradient wrote past 9 ci co'
    _all_written(dx=dx, dw=dw[:, :nw])
    e = dict(dx=0.0, dx_edge=0.0, dw=0.0)
    for k in d['checked']:
        _worse(e, 'dw', rel_err(dw[k, :nw].cpu().numpy(), _ref(name, k, 'dw').numpy()))
        if need_dx:
            _worse(e, 'dx', rel_err(dx[k].cpu().numpy(), _ref(name, k, 'dx').numpy()))
            _worse(e, 'dx_edge', _edge_err(dx[k].cpu().numpy(), _ref(name, k, 'dx')))
    if T > nd:
        for t in range(nd, T):
            assert torch.equal(dw[t, :nw], dw[t % nd, :nw]) and (not need_dx or torch.equal(dx[t], dx[t % nd])), t
        for k in range(nd):
            dx1, dw1 = run(xd[k], dzd[k], wbuf[k], 1)
            if need_dx:
                _assert_single_task(lb, form, c, 1, CS.EPI_NONE, 1, dplan, dx1[0], dx[k], k)
            assert rel_err(dw1[0, :nw].cpu().numpy(), dw[k, :nw].cpu().numpy()) < 2e-6, k
    report(f'conv_shapes_bwd[{name}|{form}]', family=wplan.family, size=wplan.size, exact=wplan.exact, **e)
    assert e['dx'] < 2e-6 and e['dx_edge'] < 2e-6 and e['dw'] < 5e-6, e


@pytest.mark.parametrize('name', NAMES)
def test_conv_tangent_shapes(lib, name):
    """zd = conv(x0, w0) + conv(x1, w1), m1 = mean zd, m2 = mean(zhat zd); the first layer (no two-term kernel) with its one term."""
    lb, form = lib
    c, d = CS.BY_NAME[name], _inputs(name)
    T, nd, ho, wo = c.T, d['nd'], d['ho'], d['wo']
    two = c.ci >= 32
    plan = _assert_conv_plan(lb, form, c, 2 if two else 1, CS.EPI_TSTATS, 0)
    x0d, x1d, zin, mud, rd = _rep(d['x0'], T), _rep(d['x1'], T), _rep(d['z'], T), _rep(d['mu'], T), _rep(d['rstd'], T)
    wbuf, (o0, o1), pstride = _weights(d, T, ['w0', 'w1'], 5)
    scratch, sb = _scratch(lb, c)

    def run(sel, tasks):
        zd, m1, m2 = _nan(tasks, c.n, ho, wo, c.co), _nan(tasks, c.co), _nan(tasks, c.co)
        _lib.check(lb.mi_conv3x3_tangent(stream(), ptr(x0d[sel]), _at(wbuf[sel], o0), ptr(x1d[sel]) if two else None,
                                         _at(wbuf[sel], o1) if two else None, pstride, ptr(zin[sel]), ptr(mud[sel]), ptr(rd[sel]), tasks,
                                         c.n, c.h, c.w, c.ci, c.co, c.stride, ptr(zd), ptr(m1), ptr(m2), ptr(scratch), sb))
        torch.cuda.synchronize()
        return zd, m1, m2

    zd, m1, m2 = run(slice(None), T)
    _all_written(zd=zd, m1=m1, m2=m2)
    e = dict(zd=0.0, zd_edge=0.0, m1=0.0, m2=0.0)
    for k in d['checked']:
        zdr = _ref(name, k, 'z') + _ref(name, k, 'z1') if two else _ref(name, k, 'z')
        zh = (_t64(d['z'][k]) - d['mu'][k].double()) * d['rstd'][k].double()
        sd = float(zdr.std())
        _worse(e, 'zd', rel_err(zd[k].cpu().numpy(), zdr.numpy()))
        _worse(e, 'zd_edge', _edge_err(zd[k].cpu().numpy(), zdr))
        _worse(e, 'm1', max_err(m1[k].cpu().numpy(), zdr.mean(dim=(0, 1, 2)).numpy()) / sd)
        _worse(e, 'm2', max_err(m2[k].cpu().numpy(), (zh * zdr).mean(dim=(0, 1, 2)).numpy()) / sd)
    if T > nd:
        for t in range(nd, T):
            assert torch.equal(zd[t], zd[t % nd]), t
            assert torch.allclose(m1[t], m1[t % nd], rtol=1e-6, atol=1e-7) and torch.allclose(m2[t], m2[t % nd], rtol=1e-6, atol=1e-7)
        for k in range(nd):
            zd1, a1, a2 = run(slice(k, k + 1), 1)
            _assert_single_task(lb, form, c, 2 if two else 1, CS.EPI_TSTATS, 0, plan, zd1[0], zd[k], k)
            assert torch.allclose(a1[0], m1[k], rtol=1e-6, atol=1e-7) and torch.allclose(a2[0], m2[k], rtol=1e-6, atol=1e-7)
    report(f'conv_shapes_tangent[{name}|{form}]', kernel=plan.kernel, tiles_per_wave=plan.tiles_per_wave, **e)
    assert e['zd'] < 2e-6 and e['zd_edge'] < 2e-6 and e['m1'] < 2e-6 and e['m2'] < 2e-6, e


@pytest.mark.parametrize('name', HIDDEN)
def test_conv_bwd_two_terms_shapes(lib, name):
    """R{dW} = wgrad(x0, dz0) + wgrad(x1, dz1) and R{dx} = dgrad(dz0, w0) + dgrad(dz1, w1)."""
    lb, form = lib
    c, d = CS.BY_NAME[name], _inputs(name)
    T, nd = c.T, d['nd']
    nw = 9 * c.ci * c.co
    wplan = _assert_wgrad_plan(lb, form, c, 2)
    dplan = _assert_conv_plan(lb, form, c, 2, CS.EPI_NONE, 1)
    x0d, x1d, d0, d1 = _rep(d['x0'], T), _rep(d['x1'], T), _rep(d['dz0'], T), _rep(d['dz1'], T)
    wbuf, (o0, o1), pstride = _weights(d, T, ['w0', 'w1'], 5)
    gstride = nw + 3
    scratch, sb = _scratch(lb, c)

    def run(sel, tasks):
        dx, dw = _nan(tasks, c.n, c.h, c.w, c.ci), _nan(tasks, gstride)
        _lib.check(lb.mi_conv3x3_bwd2(stream(), ptr(x0d[sel]), ptr(d0[sel]), ptr(x1d[sel]), ptr(d1[sel]), _at(wbuf[sel], o0), _at(wbuf[sel], o1),
                                      pstride, tasks, c.n, c.h, c.w, c.ci, c.co, c.stride, ptr(dx), ptr(dw), gstride, ptr(scratch), sb))
        torch.cuda.synchronize()
        return dx, dw

    dx, dw = run(slice(None), T)
    assert bool(torch.isnan(dw[:, nw:]).all()), 'the weight gradient wrote past 9 ci co'
    _all_written(dx=dx, dw=dw[:, :nw])
    e = dict(dx=0.0, dx_edge=0.0, dw=0.0)
    for k in d['checked']:
        _worse(e, 'dw', rel_err(dw[k, :nw].cpu().numpy(), (_ref(name, k, 'dw') + _ref(name, k, 'dw1')).numpy()))
        _worse(e, 'dx', rel_err(dx[k].cpu().numpy(), (_ref(name, k, 'dx') + _ref(name, k, 'dx1')).numpy()))
        _worse(e, 'dx_edge', _edge_err(dx[k].cpu().numpy(), _ref(name, k, 'dx') + _ref(name, k, 'dx1')))
    if T > nd:
        for t in range(nd, T):
            assert torch.equal(dw[t, :nw], dw[t % nd, :nw]) and torch.equal(dx[t], dx[t % nd]), t
        for k in range(nd):
            dx1, dw1 = run(slice(k, k + 1), 1)
            _assert_single_task(lb, form, c, 2, CS.EPI_NONE, 1, dplan, dx1[0], dx[k], k)
            assert rel_err(dw1[0, :nw].cpu().numpy(), dw[k, :nw].cpu().numpy()) < 2e-6, k
    report(f'conv_shapes_bwd2[{name}|{form}]', family=wplan.family, size=wplan.size, exact=wplan.exact,
           straddles_terms=bool(wplan.family in ('rows_f32', 'rows_bf16', 'strips_bf16') and CS.straddles_terms(wplan)), **e)
    assert e['dx'] < 2e-6 and e['dx_edge'] < 2e-6 and e['dw'] < 5e-6, e
