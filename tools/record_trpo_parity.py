"""Record tests/golden/trpo_parity_parent.npz: the inputs of every case of tests/test_gpu_trpo_parity.py and what the commit BEFORE the
one-step and the K-step TRPO implementations became one computed from them.

The fixture judges that change, so it is recorded from a build of the earlier commit, never from the code under test:

    git worktree add /tmp/before <commit> && make -C /tmp/before/exploring_meta_amd/csrc -j16
    MI_MAML_LIB=/tmp/before/exploring_meta_amd/csrc/libmi_maml.so python tools/record_trpo_parity.py [out.npz]

The earlier library still exports the one-step entry points (mi_trpo_surrogate, mi_trpo_fvp, mi_trpo_kl_prepare, mi_trpo_fvp_general);
this package no longer declares them, so their prototypes are bound here.  Cases of the `one_step` route go through them, cases of
the `steps` route through the *_steps entry points of the same library.  Needs the GPU and the oracle."""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

_P, _I, _F, _Z = C.c_void_p, C.c_int, C.c_float, C.c_size_t
ONE_STEP = {
    'mi_trpo_general_workspace_bytes': [_P, _I, _I, C.POINTER(_Z)],
    'mi_trpo_surrogate': [_P] * 13 + [_I, _I, _F, _P, _P, _P, _P, _Z],
    'mi_trpo_fvp': [_P] * 8 + [_I, _I, _F, _F, _P, _P, _P, _Z],
    'mi_trpo_kl_prepare': [_P] * 10 + [_I, _I, _F, _P, _P, _Z],
    'mi_trpo_fvp_general': [_P] * 9 + [_I, _I, _F, _F, _P, _P, _P, _Z],
}


class OneStep:
    """The earlier library's one-step entry points behind PolicyEngine's argument lists: sup [1, T, ...] is passed without its
    leading axis, and theta (which those products took) is the one of the last surrogate call."""

    def __init__(self, eng):
        import torch
        from exploring_meta_amd.engine import _ptr, _stream
        self.eng, self.torch, self.ptr, self.stream = eng, torch, _ptr, lambda: _stream(eng.device)
        for name, args in ONE_STEP.items():
            fn = getattr(eng.lib, name)                # AttributeError: MI_MAML_LIB does not point at a build of the earlier commit
            fn.restype, fn.argtypes = C.c_int, args
        self.theta = None

    def _call(self, name, T, B, *args):
        nb = _Z()
        self.eng._check(self.eng.lib.mi_trpo_general_workspace_bytes(self.eng._h, T, B, C.byref(nb)))
        if self.eng._ws is None or self.eng._ws.numel() < nb.value:
            self.eng._ws = self.torch.empty(nb.value, dtype=self.torch.uint8, device=self.eng.device)
        ws = self.eng._ws
        self.eng._check(getattr(self.eng.lib, name)(self.eng._h, self.stream(), *args, self.ptr(ws), ws.numel()))

    @staticmethod
    def _tb(sup):
        assert sup['states'].shape[0] == 1
        return sup['states'].shape[1], sup['states'].shape[2]

    def _new(self, n=None):
        return self.torch.empty(self.eng.param_count if n is None else n, device=self.eng.device)

    def surrogate(self, theta, sup, qry, old_loc, old_scale, inner_lr, want_grad):
        (T, B), p, self.theta = self._tb(sup), self.ptr, theta.contiguous()
        loss, kl, grad = self._new(1), self._new(1), self._new() if want_grad else None
        self._call('mi_trpo_surrogate', T, B, p(self.theta), p(sup['states']), p(sup['actions']), p(sup['adv']), p(sup['count']),
                   p(qry['states']), p(qry['actions']), p(qry['adv']), p(qry['count']), p(old_loc), p(old_scale), T, B,
                   float(inner_lr), p(loss), p(kl), p(grad))
        return loss, kl, grad

    def fvp(self, sup, qry, inner_lr, damping, v):
        (T, B), p, out = self._tb(sup), self.ptr, self._new()
        self._call('mi_trpo_fvp', T, B, p(self.theta), p(sup['states']), p(sup['actions']), p(sup['count']), p(qry['states']),
                   p(qry['count']), T, B, float(inner_lr), float(damping), p(v.contiguous()), p(out))
        return out

    def kl_prepare(self, sup, qry, old_loc, old_scale, inner_lr, want_grad=False):
        (T, B), p, grad = self._tb(sup), self.ptr, self._new() if want_grad else None
        self._call('mi_trpo_kl_prepare', T, B, p(self.theta), p(sup['states']), p(sup['actions']), p(sup['count']), p(qry['states']),
                   p(qry['count']), p(old_loc), p(old_scale), T, B, float(inner_lr), p(grad))
        return grad

    def fvp_general(self, sup, qry, old_scale, inner_lr, damping, v):
        (T, B), p, out = self._tb(sup), self.ptr, self._new()
        self._call('mi_trpo_fvp_general', T, B, p(self.theta), p(sup['states']), p(sup['actions']), p(sup['count']), p(qry['states']),
                   p(qry['count']), p(old_scale), T, B, float(inner_lr), float(damping), p(v.contiguous()),
                   p(out))
        return out


def main():
    import trpo_parity_cases as TP
    out = sys.argv[1] if len(sys.argv) > 1 else TP.FIXTURE
    arrays = TP.build_inputs()
    np.savez(out + '.inputs.npz', **arrays)                    # the cases read their inputs the way the test will
    npz = np.load(out + '.inputs.npz')
    for case, (name, route, _, fn, kw) in TP.CASES.items():
        eng = TP.engine(name)
        got = fn(OneStep(eng) if route == 'one_step' else eng, TP.load_inputs(npz, name), **kw)
        for k, v in got.items():
            arrays[f'{case}/out/{k}'] = v.cpu().numpy()
        print(case, route, {k: (float(v) if v.numel() == 1 else tuple(v.shape)) for k, v in got.items()})
    os.remove(out + '.inputs.npz')
    assert all(np.isfinite(a).all() for a in arrays.values())
    np.savez_compressed(out, **arrays)
    print(f'{len(arrays)} arrays -> {out}: {os.path.getsize(out)} bytes (library: {os.environ.get("MI_MAML_LIB", "in-tree")})')


if __name__ == '__main__':
    main()
