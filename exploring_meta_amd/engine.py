"""Batched MAML engine: Python host over the C ABI (include/mi_maml.h).

``MetaEngine.meta_batch`` processes a whole meta-batch of tasks in one call -- what the reference does with a sequential
Python loop of ``maml.clone()`` / ``fast_adapt`` / ``eval_loss.backward()`` (vision/maml_vision.py:102-114).  PyTorch is
used only for device memory and streams; all arithmetic runs in libmi_maml's HIP kernels.
"""

import ctypes as C
import math
from dataclasses import dataclass

import torch

from . import _lib


@dataclass(frozen=True)
class ModelSpec:
    """Architecture of the reference's few-shot classifiers (core_functions/vision_models.py)."""
    n_layers: int
    in_channels: int
    in_h: int
    in_w: int
    hidden: int
    max_pool: bool
    ways: int
    head_mean_pool: bool

    @staticmethod
    def mini_imagenet(ways, hidden=32, layers=4):
        """MiniImagenetCNN(output_size=ways, hidden_size=32, layers=4) (vision_models.py:93-105)."""
        return ModelSpec(layers, 3, 84, 84, hidden, True, ways, False)

    @staticmethod
    def omniglot(ways, hidden=64, layers=4):
        """OmniglotCNN(output_size=ways, hidden_size=64, layers=4) (vision_models.py:39-49)."""
        return ModelSpec(layers, 1, 28, 28, hidden, False, ways, True)

    @staticmethod
    def anil(ways, hidden=64, channels=3, max_pool=True, layers=4, in_hw=84):
        """ANIL trunk ConvBase(output_size, hidden, channels, max_pool) + Linear(fc_neurons, ways) head
        (vision/anil_vision.py:86-94): Mini-ImageNet (64 filters, 3x84x84, pooling) or Omniglot (32 filters, 1x28x28)."""
        return ModelSpec(layers, channels, in_hw, in_hw, hidden, bool(max_pool), ways, False)

    def block_output_shape(self, layer):
        """(C, H, W) after the first `layer` ConvBlocks (layer in 1..n_layers)."""
        if not 1 <= layer <= self.n_layers:
            raise ValueError(f'layer must be in 1..{self.n_layers}')
        h, w = self.in_h, self.in_w
        for _ in range(layer):
            if self.max_pool:
                h, w = h // 2, w // 2
            else:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        return self.hidden, h, w

    def param_shapes(self):
        """(name, shape) in the reference's parameters() order / state_dict naming."""
        out, ci = [], self.in_channels
        for i in range(self.n_layers):
            out += [(f'base.{i}.normalize.weight', (self.hidden,)), (f'base.{i}.normalize.bias', (self.hidden,)),
                    (f'base.{i}.conv.weight', (self.hidden, ci, 3, 3)), (f'base.{i}.conv.bias', (self.hidden,))]
            ci = self.hidden
        h, w = self.in_h, self.in_w
        for _ in range(self.n_layers):
            if self.max_pool:
                h, w = h // 2, w // 2
            else:
                h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        feat = self.hidden if self.head_mean_pool else self.hidden * h * w
        out += [('linear.weight', (self.ways, feat)), ('linear.bias', (self.ways,))]
        return out


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _on_device(fn):
    """Run an engine method with the engine's own device current (launches go to that device's current stream), whatever
    device the caller has selected."""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *args, **kwargs):
        with torch.cuda.device(self.device):
            return fn(self, *args, **kwargs)
    return wrapped


def _resolve_device(device):
    if device is None:
        return torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise _lib.MiError(f'the engine runs on a GPU, got device {device}')
    return torch.device('cuda', device.index if device.index is not None else torch.cuda.current_device())


METRICS = {'proto': 0, 'cosine': 1}          # MI_METRIC_PROTO, MI_METRIC_COSINE (include/mi_maml.h)


def metric_id(metric):
    """The library's id of a metric head; anything else is refused here, before the library is touched."""
    if metric not in METRICS:
        raise _lib.MiError(f"libmi_maml error -1: unknown metric {metric!r}: 'proto' (Prototypical Networks) or 'cosine' (NIL)")
    return METRICS[metric]


def check_scale(scale):
    scale = float(scale)
    if not scale > 0.0:
        raise _lib.MiError(f'libmi_maml error -1: the metric head\'s scale must be positive, got {scale}')
    return scale


def check_ridge(lam, scale):
    """(lam, scale) of the ridge head as floats; anything not > 0 or not finite is refused here, before the library is touched."""
    lam, scale = float(lam), float(scale)
    for name, v in (('lam', lam), ('scale', scale)):
        if not (v > 0.0 and math.isfinite(v)):
            raise _lib.MiError(f'libmi_maml error -1: the ridge head\'s {name} must be positive and finite, got {v}')
    return lam, scale


def check_logreg(lam, scale):
    """(lam, scale) of the logistic-regression head as floats; anything not > 0 or not finite is refused here, before the library is touched."""
    lam, scale = float(lam), float(scale)
    for name, v in (('lam', lam), ('scale', scale)):
        if not (v > 0.0 and math.isfinite(v)):
            raise _lib.MiError(f'libmi_maml error -1: the logistic-regression head\'s {name} must be positive and finite, got {v}')
    return lam, scale


class MetaEngine:
    """One engine per (model spec, device).  Not re-entrant (one host thread per GPU / rank)."""

    def __init__(self, spec, device=None):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MiError('MetaEngine needs a GPU: the MAML hot path has no CPU implementation in this package '
                               '(the CPU restatement under oracle/ is test infrastructure only).')
        self.spec = spec
        self.device = _resolve_device(device)
        desc = _lib.MiModelDesc(spec.n_layers, spec.in_channels, spec.in_h, spec.in_w, spec.hidden, int(spec.max_pool),
                                spec.ways, int(spec.head_mean_pool))
        self._h = C.c_void_p()
        _lib.check(self.lib.mi_engine_create(C.byref(desc), self.device.index, C.byref(self._h)))
        n = C.c_size_t()
        _lib.check(self.lib.mi_param_count(self._h, C.byref(n)), self._h)
        self.param_count = n.value
        self._ws = None

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.mi_engine_destroy(h)
            self._h = C.c_void_p()

    def set_fused_block1(self, on):
        """Ablation/test switch for the conv-recompute kernels of block 1: 0 generic kernels, 1 (default) fused kernels with the Gram-matrix path for
        the support passes and the query pass, 2 fused kernels without it, 3 the Gram-matrix path for the support passes only."""
        _lib.check(self.lib.mi_engine_set_fused_block1(self._h, int(on)), self._h)

    def set_overlap(self, on):
        """Side-stream execution of the weight gradients of blocks >= 2 (default on: one fork of the side stream per hidden block; any
        non-zero value means on); results do not depend on it."""
        _lib.check(self.lib.mi_engine_set_overlap(self._h, int(on)), self._h)

    def set_fused_finalize(self, on):
        """BatchNorm partials folded inside the producing kernels (default on) or by separate launches; bit-identical results."""
        _lib.check(self.lib.mi_engine_set_fused_finalize(self._h, int(on)), self._h)

    def set_fused_block1_reduce(self, on):
        """Block 1's BatchNorm-backward sums in the epilogue of block 2's dgrad (default on) or as a separate streaming pass."""
        _lib.check(self.lib.mi_engine_set_fused_block1_reduce(self._h, int(on)), self._h)

    def set_fused_tail(self, on):
        """One "advance" launch at the end of every pass of `meta_batch` (default on) or the separate fold / update / statistics
        launches; bit-identical results."""
        _lib.check(self.lib.mi_engine_set_fused_tail(self._h, int(on)), self._h)

    def set_fused_last_block(self, on):
        """The last block's BatchNorm + pooling, the head, its backward and that block's BatchNorm backward (or their tangents) as one launch
        per pass with one workgroup per task (default on) or the five separate launches (mi_engine_set_fused_last_block)."""
        _lib.check(self.lib.mi_engine_set_fused_last_block(self._h, int(on)), self._h)

    def set_graph(self, on):
        """Replay repeated identical fused calls as one hipGraphLaunch (mi_engine_set_graph).  While on, `meta_batch` /
        `meta_batch_anil` return views of PERSISTENT output buffers (one set per call shape), because a replay writes where the
        captured call wrote: results are valid until the next call of the same shape; copy what must outlive it.  The caller keeps
        theta / data / labels in place between iterations (in-place optimizer step, resident task batches) to benefit."""
        _lib.check(self.lib.mi_engine_set_graph(self._h, int(on)), self._h)
        self._graph = bool(on)
        self._persist = {}
        # stream capture is not permitted on the legacy default stream torch hands out as "current": graph-mode calls run on an
        # engine-owned stream, ordered after / before the caller's current stream with events
        self._gstream = torch.cuda.Stream(device=self.device) if on else None

    def _fused_call(self, fn, *args):
        """Issue one fused C call on the caller's current stream, or (graph mode) on the engine's capture-capable stream, fenced
        against the current stream on both sides."""
        gs = getattr(self, '_gstream', None)
        if gs is None:
            return fn(self._h, _stream(self.device), *args)
        cur = torch.cuda.current_stream(self.device)
        gs.wait_stream(cur)
        rc = fn(self._h, C.c_void_p(gs.cuda_stream), *args)
        cur.wait_stream(gs)
        return rc

    def _persistent(self, key, make):
        """make(): fresh tensors, or (graph mode, where a replay writes where the captured call wrote) the persistent ones under `key`."""
        if not getattr(self, '_graph', False):
            return make()
        if key not in self._persist:
            self._persist[key] = make()
        return self._persist[key]

    def _outputs(self, kind, T, nlog, with_grad, return_logits):
        """(loss, acc, grad, logits) buffers of one fused call: fresh tensors, or the persistent set of this shape in graph mode."""
        def fresh():
            # one allocation [grad (P) | loss (T) | acc (T)]: a data-parallel caller all-reduces the three as ONE contiguous buffer
            # (sharding.MetaTrainer) without gathering them into a new tensor first
            P = self.param_count if with_grad else 0
            buf = torch.empty(P + 2 * T, dtype=torch.float32, device=self.device)
            return (buf[P:P + T], buf[P + T:], buf[:P] if with_grad else None,
                    torch.empty(T, nlog, self.spec.ways, dtype=torch.float32, device=self.device) if return_logits else None)
        return self._persistent((kind, T, nlog, bool(with_grad), bool(return_logits)), fresh)

    def set_bn_export(self, tasks=0, passes=0):
        """mi_engine_set_bn_export: while on, every fused call also leaves the BatchNorm batch statistics of each of its forward
        passes in the returned tensor [passes, tasks, 2, C_total] (mean, biased variance; C_total = blocks x filters, block-major).
        passes = adapt_steps + 1 for meta_batch (inner steps, then the query pass), 1 for meta_batch_anil.  tasks = 0 switches it off."""
        if not tasks:
            _lib.check(self.lib.mi_engine_set_bn_export(self._h, C.c_void_p(0), 0), self._h)
            self._bn_export = None
            return None
        ctot = self.spec.hidden * self.spec.n_layers
        self._bn_export = torch.zeros(passes, tasks, 2, ctot, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_engine_set_bn_export(self._h, _ptr(self._bn_export), self._bn_export.numel()), self._h)
        return self._bn_export

    def set_trace(self, tasks=0, adapt_steps=0):
        """Debug/test aid (mi_debug_set_trace): allocate a trace buffer for meta_batch calls with these sizes and return it as a
        dict of views {theta [K+1,T,P], g [K,T,P], lam_in [K,T,P], hv [K,T,P]} (reference parameter order); 0 tasks switches it off."""
        if not tasks:
            _lib.check(self.lib.mi_debug_set_trace(self._h, None, 0), self._h)
            self._trace = None
            return None
        K, T, P = adapt_steps, tasks, self.param_count
        buf = torch.zeros((4 * K + 1) * T * P, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_debug_set_trace(self._h, _ptr(buf), buf.numel()), self._h)
        self._trace = buf
        v = buf.view(4 * K + 1, T, P)
        return dict(theta=v[:K + 1], g=v[K + 1:2 * K + 1], lam_in=v[2 * K + 1:3 * K + 1], hv=v[3 * K + 1:])

    def workspace_bytes(self, tasks, shots, adapt_steps, second_order):
        b = C.c_size_t()
        _lib.check(self.lib.mi_workspace_bytes(self._h, tasks, self.spec.ways, shots, adapt_steps, int(second_order),
                                               C.byref(b)), self._h)
        return b.value

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = None
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _check_batch(self, theta, data, labels, shots, lr_vec=None, flat_data=True):
        """Shapes, dtypes and contiguity of a fused call's tensors; returns T.  flat_data: one-channel images may come without the
        channel axis."""
        s = self.spec
        T = data.shape[0]
        n2 = 2 * shots * s.ways
        if tuple(data.shape) != (T, n2, s.in_channels, s.in_h, s.in_w) and \
                not (flat_data and s.in_channels == 1 and data.numel() == T * n2 * s.in_h * s.in_w):
            raise ValueError(f'data shape {tuple(data.shape)} does not match [T, {n2}, {s.in_channels}, {s.in_h}, {s.in_w}]')
        if tuple(labels.shape) != (T, n2):
            raise ValueError(f'labels shape {tuple(labels.shape)} != {(T, n2)}')
        if theta.numel() != self.param_count:
            raise ValueError(f'theta has {theta.numel()} elements, the model has {self.param_count}')
        for t, dt in ((theta, torch.float32), (data, torch.float32), (labels, torch.int64)) + (((lr_vec, torch.float32),) if lr_vec is not None else ()):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError('theta/data/lr_vec must be contiguous fp32 CUDA tensors and labels contiguous int64 CUDA')
        return T

    def _maml_call(self, theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, grad_tasks, want_lr_grad, return_logits,
                   step_w=None, offsets=None, want_offsets_grad=False):
        """mi_meta_batch_maml_tv, or mi_meta_batch_maml_lr when the step sizes are a vector, or -- step_w given -- mi_meta_batch_maml_steps
        with either kind of step (loss, acc and logits then carry a leading axis of adapt_steps + 1).  Returns (loss, acc, grad, lr_grad, logits).
        offsets given: mi_meta_batch_maml_offsets with any of those forms, and offsets_grad as a sixth result."""
        s = self.spec
        T = self._check_batch(theta, data, labels, shots, lr_vec)
        if offsets is not None:
            # the library reads adapt_steps * P floats at offsets on the device: anything else is refused here, before any launch
            if adapt_steps < 1:
                raise _lib.MiError('libmi_maml error -1: meta_batch_offsets needs adapt_steps >= 1')
            if not torch.is_tensor(offsets) or offsets.dtype != torch.float32 or not offsets.is_cuda or offsets.device != theta.device or \
                    not offsets.is_contiguous() or tuple(offsets.shape) != (adapt_steps, self.param_count):
                raise _lib.MiError(f'libmi_maml error -1: offsets must be a contiguous fp32 tensor of shape ({adapt_steps}, {self.param_count}) '
                                   f'on {theta.device}')
            if want_offsets_grad and grad_tasks == 0:
                raise _lib.MiError('libmi_maml error -1: offsets_grad wanted but grad_tasks = 0: the offset gradient is summed over the train tasks')
        if step_w is not None:
            # the library reads adapt_steps floats at step_w on the device: anything else is refused here, before any launch
            if adapt_steps < 1:
                raise _lib.MiError('libmi_maml error -1: meta_batch_steps needs adapt_steps >= 1')
            if not torch.is_tensor(step_w) or step_w.dtype != torch.float32 or not step_w.is_cuda or step_w.device != theta.device or \
                    not step_w.is_contiguous() or tuple(step_w.shape) != (adapt_steps,):
                raise _lib.MiError(f'libmi_maml error -1: step_w must be a contiguous fp32 tensor of shape ({adapt_steps},) on {theta.device}')
        if lr_vec is not None:
            # the library sizes its reads of lr_vec from lr_steps and P: a buffer of another size is refused here, before any launch
            if lr_vec.numel() % self.param_count != 0 or lr_vec.numel() == 0 or lr_vec.dim() > 2 or \
                    (lr_vec.dim() == 2 and lr_vec.shape[1] != self.param_count):
                raise _lib.MiError(f'libmi_maml error -1: lr_vec has shape {tuple(lr_vec.shape)}, expected [P], [1, P] or [adapt_steps, P] '
                                   f'with P = {self.param_count}')
            lr_steps = lr_vec.numel() // self.param_count
        if not 0 <= grad_tasks <= T:
            raise ValueError(f'grad_tasks must be in 0..{T}, got {grad_tasks}')
        with_grad = grad_tasks > 0
        so = (not first_order) and with_grad
        b = C.c_size_t(0 if lr_vec is not None or step_w is not None or offsets is not None else self.workspace_bytes(T, shots, adapt_steps, so))
        if offsets is not None:
            if self.lib.mi_workspace_bytes_offsets(self._h, T, int(grad_tasks), s.ways, shots, adapt_steps, int(so),
                                                   lr_steps if lr_vec is not None else 0, int(bool(want_lr_grad)), int(step_w is not None),
                                                   C.byref(b)):
                raise _lib.MiError(f'libmi_maml error -1: lr_steps must be 1 or adapt_steps = {adapt_steps}')
            return self._offsets_call(theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, grad_tasks, want_lr_grad,
                                      return_logits, step_w, offsets, want_offsets_grad, T, self._workspace(b.value))
        if step_w is not None:
            if self.lib.mi_workspace_bytes_steps(self._h, T, int(grad_tasks), s.ways, shots, adapt_steps, int(so),
                                                 lr_steps if lr_vec is not None else 0, int(bool(want_lr_grad)), C.byref(b)):
                raise _lib.MiError(f'libmi_maml error -1: lr_steps must be 1 or adapt_steps = {adapt_steps}')
        elif lr_vec is not None and self.lib.mi_workspace_bytes_lr(self._h, T, s.ways, shots, adapt_steps, int(so), lr_steps,
                                                                 int(bool(want_lr_grad)), C.byref(b)):
            raise _lib.MiError(f'libmi_maml error -1: lr_steps = {lr_steps} must be 1 or adapt_steps = {adapt_steps}')
        ws = self._workspace(b.value)
        if step_w is not None:
            return self._steps_call(theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, grad_tasks, want_lr_grad,
                                    return_logits, step_w, T, ws)
        loss, acc, grad, logits = self._outputs('maml' if lr_vec is None else 'maml_lr', T, shots * s.ways, with_grad, return_logits)
        head = (_ptr(theta), _ptr(data), _ptr(labels), T, int(grad_tasks), s.ways, shots, adapt_steps)
        tail = (_ptr(logits), _ptr(ws), ws.numel())
        lr_grad = None
        if lr_vec is None:
            rc = self._fused_call(self.lib.mi_meta_batch_maml_tv, *head, float(inner_lr), int(not first_order), _ptr(loss), _ptr(acc), _ptr(grad),
                                  *tail)
        else:
            if want_lr_grad:
                lr_grad = self._persistent(('lr_grad', T, lr_steps),
                                           lambda: torch.empty(lr_steps, self.param_count, dtype=torch.float32, device=self.device))
            rc = self._fused_call(self.lib.mi_meta_batch_maml_lr, *head, _ptr(lr_vec), lr_steps, int(not first_order), _ptr(loss), _ptr(acc),
                                  _ptr(grad), _ptr(lr_grad), *tail)
        _lib.check(rc, self._h)
        return loss, acc, grad, lr_grad, logits

    def _steps_call(self, theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, grad_tasks, want_lr_grad, return_logits,
                    step_w, T, ws):
        """The C call of `_maml_call` for mi_meta_batch_maml_steps: per-step outputs [adapt_steps + 1, T, ...]."""
        s, K1 = self.spec, adapt_steps + 1
        with_grad = grad_tasks > 0
        lr_steps = 0 if lr_vec is None else lr_vec.numel() // self.param_count

        def fresh():
            return (torch.empty(K1, T, dtype=torch.float32, device=self.device), torch.empty(K1, T, dtype=torch.float32, device=self.device),
                    torch.empty(self.param_count, dtype=torch.float32, device=self.device) if with_grad else None,
                    torch.empty(K1, T, shots * s.ways, s.ways, dtype=torch.float32, device=self.device) if return_logits else None)
        loss, acc, grad, logits = self._persistent(('steps', lr_vec is None, K1, T, shots * s.ways, with_grad, bool(return_logits)), fresh)
        lr_grad = None
        if lr_vec is not None and want_lr_grad:
            lr_grad = self._persistent(('lr_grad_steps', T, lr_steps),
                                       lambda: torch.empty(lr_steps, self.param_count, dtype=torch.float32, device=self.device))
        rc = self._fused_call(self.lib.mi_meta_batch_maml_steps, _ptr(theta), _ptr(data), _ptr(labels), T, int(grad_tasks), s.ways, shots,
                              adapt_steps, float(inner_lr) if lr_vec is None else 0.0, _ptr(lr_vec), lr_steps, _ptr(step_w),
                              int(not first_order), _ptr(loss), _ptr(acc), _ptr(grad), _ptr(lr_grad), _ptr(logits), _ptr(ws), ws.numel())
        _lib.check(rc, self._h)
        return loss, acc, grad, lr_grad, logits

    def _offsets_call(self, theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, grad_tasks, want_lr_grad, return_logits,
                      step_w, offsets, want_offsets_grad, T, ws):
        """The C call of `_maml_call` for mi_meta_batch_maml_offsets: the plain outputs [T, ...], or with step_w [adapt_steps + 1, T, ...]."""
        s = self.spec
        lead = () if step_w is None else (adapt_steps + 1,)
        with_grad = grad_tasks > 0
        lr_steps = 0 if lr_vec is None else lr_vec.numel() // self.param_count
        P = self.param_count

        def fresh():
            return (torch.empty(*lead, T, dtype=torch.float32, device=self.device), torch.empty(*lead, T, dtype=torch.float32, device=self.device),
                    torch.empty(P, dtype=torch.float32, device=self.device) if with_grad else None,
                    torch.empty(*lead, T, shots * s.ways, s.ways, dtype=torch.float32, device=self.device) if return_logits else None)
        loss, acc, grad, logits = self._persistent(('offsets', lr_vec is None, lead, adapt_steps, T, shots * s.ways, with_grad, bool(return_logits)),
                                                   fresh)
        lr_grad = offsets_grad = None
        if lr_vec is not None and want_lr_grad:
            lr_grad = self._persistent(('lr_grad_offsets', T, lr_steps), lambda: torch.empty(lr_steps, P, dtype=torch.float32, device=self.device))
        if want_offsets_grad:
            offsets_grad = self._persistent(('offsets_grad', T, adapt_steps),
                                            lambda: torch.empty(adapt_steps, P, dtype=torch.float32, device=self.device))
        rc = self._fused_call(self.lib.mi_meta_batch_maml_offsets, _ptr(theta), _ptr(data), _ptr(labels), T, int(grad_tasks), s.ways, shots,
                              adapt_steps, float(inner_lr) if lr_vec is None else 0.0, _ptr(lr_vec), lr_steps, _ptr(step_w), _ptr(offsets),
                              int(not first_order), _ptr(loss), _ptr(acc), _ptr(grad), _ptr(lr_grad), _ptr(offsets_grad), _ptr(logits), _ptr(ws),
                              ws.numel())
        _lib.check(rc, self._h)
        return loss, acc, grad, lr_grad, logits, offsets_grad

    @_on_device
    def meta_batch_offsets(self, theta, data, labels, shots, adapt_steps, offsets, inner_lr=None, lr_vec=None, step_w=None, first_order=False,
                           grad_tasks=None, want_lr_grad=False, want_offsets_grad=False, return_logits=False):
        """`meta_batch` / `meta_batch_lr` / `meta_batch_steps` with per-step parameter offsets (mi_meta_batch_maml_offsets): inner step k
        ends in theta_{k+1} = (theta_k - D_k g_k) + offsets[k].  offsets [adapt_steps, P] contiguous fp32 on the engine's device,
        parameters() order, shared by the tasks; its values are read on the device by every call, graph replays included.  inner_lr (a
        number) or lr_vec; step_w None: the plain objective and outputs [T, ..], else the multi-step loss and outputs [K + 1, T, ..].
        Returns (loss, acc, meta_grad [P] or None, lr_grad or None, offsets_grad [adapt_steps, P] or None, logits or None);
        offsets_grad (``want_offsets_grad``) is the gradient of the train tasks' summed objective with respect to offsets."""
        if (inner_lr is None) == (lr_vec is None):
            raise ValueError('meta_batch_offsets takes exactly one of inner_lr and lr_vec')
        if offsets is None:
            raise ValueError('meta_batch_offsets needs offsets [adapt_steps, P]')
        loss, acc, grad, lr_grad, logits, offsets_grad = self._maml_call(
            theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order, data.shape[0] if grad_tasks is None else grad_tasks,
            want_lr_grad, return_logits, step_w=step_w, offsets=offsets, want_offsets_grad=want_offsets_grad)
        return loss, acc, grad, lr_grad, offsets_grad, logits

    @_on_device
    def meta_batch_steps(self, theta, data, labels, shots, adapt_steps, step_w, inner_lr=None, lr_vec=None, first_order=False, grad_tasks=None,
                         want_lr_grad=False, return_logits=False):
        """`meta_batch` / `meta_batch_lr` with the query set scored after 0, 1, .., adapt_steps inner steps in the one call, and the
        multi-step loss sum_j step_w[j - 1] * L_query(theta_j) as the outer objective (mi_meta_batch_maml_steps).  step_w [adapt_steps]
        fp32 on the engine's device, read there by every call, graph replays included: annealing it in place recaptures nothing.
        inner_lr (a number) or lr_vec (as in `meta_batch_lr`).  grad_tasks = None: every task is a train task; 0: evaluation only.
        Returns (loss [K + 1, T], acc [K + 1, T], meta_grad [P] or None, lr_grad or None, logits [K + 1, T, S*W, ways] or None)."""
        if (inner_lr is None) == (lr_vec is None):
            raise ValueError('meta_batch_steps takes exactly one of inner_lr and lr_vec')
        return self._maml_call(theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, first_order,
                               data.shape[0] if grad_tasks is None else grad_tasks, want_lr_grad, return_logits, step_w=step_w)

    @_on_device
    def meta_batch(self, theta, data, labels, shots, adapt_steps, inner_lr, first_order=False, with_grad=True,
                   return_logits=False, grad_tasks=None):
        """theta [P] fp32; data [T, 2*shots*ways, C, H, W] fp32 (the reference's task batches, stacked); labels [T, 2*S*W]
        int64.  Returns (loss[T], acc[T], meta_grad[P] summed over tasks or None, logits [T, S*W, ways] or None).
        grad_tasks = G (0 < G < T): the first G tasks are the meta-iteration's TRAIN tasks (the meta-gradient is summed over them), the
        other T - G its VALIDATION tasks, adapted and scored in the same launches without a backward half (maml_vision.py:117-124)."""
        if grad_tasks is None:
            grad_tasks = data.shape[0] if with_grad else 0
        loss, acc, grad, _, logits = self._maml_call(theta, data, labels, shots, adapt_steps, inner_lr, None, first_order, grad_tasks, False,
                                                     return_logits)
        return loss, acc, grad, logits

    @_on_device
    def meta_batch_lr(self, theta, data, labels, shots, adapt_steps, lr_vec, first_order=False, grad_tasks=None, want_lr_grad=False,
                      return_logits=False):
        """`meta_batch` with one inner-loop step size per parameter (mi_meta_batch_maml_lr): lr_vec [P] or [1, P] (one vector for every
        inner step) or [adapt_steps, P] (one per step), fp32 on the engine's device, parameters() order.  Its values are read on the
        device by every call, graph replays included.  grad_tasks = None: every task is a train task; 0: evaluation only.
        Returns (loss[T], acc[T], meta_grad[P] or None, lr_grad [lr_steps, P] or None, logits or None); lr_grad (``want_lr_grad``) is
        the gradient of the summed query loss of the train tasks with respect to lr_vec."""
        return self._maml_call(theta, data, labels, shots, adapt_steps, None, lr_vec, first_order,
                               data.shape[0] if grad_tasks is None else grad_tasks, want_lr_grad, return_logits)

    @_on_device
    def meta_batch_anil(self, theta, data, labels, shots, adapt_steps, inner_lr, first_order=False, with_grad=True,
                        return_logits=False):
        """ANIL (reference vision/anil_vision.py:116-122): theta = [features.parameters()..., head.weight, head.bias] flat;
        the trunk sees all 2*shots*ways images of a task at once, only the head is adapted.  Same returns as meta_batch."""
        s = self.spec
        T = self._check_batch(theta, data, labels, shots, flat_data=False)
        b = C.c_size_t()
        _lib.check(self.lib.mi_anil_workspace_bytes(self._h, T, s.ways, shots, adapt_steps, C.byref(b)), self._h)
        ws = self._workspace(b.value)
        loss, acc, grad, logits = self._outputs('anil', T, shots * s.ways, with_grad, return_logits)
        rc = self._fused_call(self.lib.mi_meta_batch_anil, _ptr(theta), _ptr(data), _ptr(labels), T, s.ways, shots,
                              adapt_steps, float(inner_lr), int(not first_order), int(with_grad), _ptr(loss),
                              _ptr(acc), _ptr(grad), _ptr(logits), _ptr(ws), ws.numel())
        _lib.check(rc, self._h)
        return loss, acc, grad, logits

    def head_param_count(self):
        """Ph = ways * fc_neurons + ways: the entries of the ANIL head (the last two tensors of `param_shapes`)."""
        (_, ws), (_, bs) = self.spec.param_shapes()[-2:]
        return ws[0] * ws[1] + bs[0]

    def _anil_call(self, theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, step_w, first_order, with_grad, want_lr_grad, return_logits,
                   proto_scale=None):
        """mi_meta_batch_anil_lr (step_w None) or mi_meta_batch_anil_steps (loss, acc and logits then carry a leading axis of
        adapt_steps + 1).  Returns (loss, acc, grad, lr_grad, logits).  proto_scale: mi_meta_batch_anil_proto with that scale (scalar or
        vector step, with or without step_w); the per-task scale gradient [T] (None without a gradient) then comes before logits."""
        s, K, Ph = self.spec, int(adapt_steps), self.head_param_count()
        T = self._check_batch(theta, data, labels, shots, flat_data=False)
        steps, proto = step_w is not None, proto_scale is not None

        def refuse(name, t, shape_text, ok_shape):
            # the library sizes its reads of lr_vec / step_w from the call's integers: anything else is refused here, before any launch
            if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_cuda or t.device != theta.device or not t.is_contiguous() or \
                    not ok_shape:
                shape = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
                raise _lib.MiError(f'libmi_maml error -1: {name} must be a contiguous fp32 tensor of shape {shape_text} on {theta.device}, '
                                   f'got {shape}')
        if steps:
            if K < 1:
                raise _lib.MiError(f'libmi_maml error -1: meta_batch_anil_steps needs adapt_steps >= 1, got {K}')
            refuse('step_w', step_w, f'({K},)', torch.is_tensor(step_w) and tuple(step_w.shape) == (K,))
        lr_steps = 0
        if lr_vec is not None:
            ok = torch.is_tensor(lr_vec) and lr_vec.dim() in (1, 2) and lr_vec.shape[-1] == Ph and \
                (lr_vec.dim() == 1 or lr_vec.shape[0] in (1, max(K, 1)))
            refuse('lr_vec', lr_vec, f'[{Ph}], [1, {Ph}] or [{max(K, 1)}, {Ph}] (Ph = ways * fc_neurons + ways)', ok)
            lr_steps = lr_vec.numel() // Ph
        so = (not first_order) and with_grad
        want_lr_grad = bool(want_lr_grad) and lr_vec is not None and bool(with_grad)
        b = C.c_size_t()
        _lib.check((self.lib.mi_anil_proto_workspace_bytes if proto else self.lib.mi_anil_workspace_bytes_steps)(self._h, T, s.ways, shots, K, int(bool(with_grad)), int(so), lr_steps,
                                                          int(want_lr_grad), int(steps), C.byref(b)), self._h)
        ws = self._workspace(b.value)
        nlog = shots * s.ways
        if steps:
            def fresh():
                return (torch.empty(K + 1, T, dtype=torch.float32, device=self.device), torch.empty(K + 1, T, dtype=torch.float32, device=self.device),
                        torch.empty(self.param_count, dtype=torch.float32, device=self.device) if with_grad else None,
                        torch.empty(K + 1, T, nlog, s.ways, dtype=torch.float32, device=self.device) if return_logits else None)
            loss, acc, grad, logits = self._persistent(('anil_steps', proto, lr_vec is None, K + 1, T, nlog, bool(with_grad), bool(return_logits)), fresh)
        else:
            loss, acc, grad, logits = self._outputs('anil_proto' if proto else 'anil_lr', T, nlog, with_grad, return_logits)
        lr_grad = None
        if want_lr_grad:
            lr_grad = self._persistent(('anil_lr_grad', proto, steps, T, lr_steps), lambda: torch.empty(lr_steps, Ph, dtype=torch.float32, device=self.device))
        head = (_ptr(theta), _ptr(data), _ptr(labels), T, s.ways, shots, K)
        tail = (_ptr(loss), _ptr(acc), _ptr(grad), _ptr(lr_grad), _ptr(logits), _ptr(ws), ws.numel())
        if proto:
            dscale = self._persistent(('anil_proto_dscale', steps, T), lambda: torch.empty(T, dtype=torch.float32, device=self.device)) if with_grad else None
            rc = self._fused_call(self.lib.mi_meta_batch_anil_proto, *head, int(not first_order), float(inner_lr) if lr_vec is None else 0.0,
                                  _ptr(lr_vec), lr_steps, _ptr(step_w), proto_scale, int(bool(with_grad)), _ptr(loss), _ptr(acc), _ptr(grad),
                                  _ptr(lr_grad), _ptr(dscale), _ptr(logits), _ptr(ws), ws.numel())
            _lib.check(rc, self._h)
            return loss, acc, grad, lr_grad, dscale, logits
        if steps:
            rc = self._fused_call(self.lib.mi_meta_batch_anil_steps, *head, float(inner_lr) if lr_vec is None else 0.0, _ptr(lr_vec), lr_steps,
                                  _ptr(step_w), int(not first_order), int(bool(with_grad)), *tail)
        else:
            rc = self._fused_call(self.lib.mi_meta_batch_anil_lr, *head, _ptr(lr_vec), lr_steps, int(not first_order), int(bool(with_grad)), *tail)
        _lib.check(rc, self._h)
        return loss, acc, grad, lr_grad, logits

    @_on_device
    def meta_batch_anil_lr(self, theta, data, labels, shots, adapt_steps, lr_vec, first_order=False, with_grad=True, want_lr_grad=False,
                           return_logits=False):
        """`meta_batch_anil` with one inner-loop step size per head parameter (mi_meta_batch_anil_lr): lr_vec [Ph], [1, Ph] or
        [adapt_steps, Ph] with Ph = ways * fc_neurons + ways, fp32 on the engine's device, in the order of ``head.parameters()`` (weight,
        bias).  Its values are read on the device by every call, graph replays included.
        Returns (loss[T], acc[T], meta_grad[P] or None, lr_grad [lr_steps, Ph] or None, logits or None)."""
        if lr_vec is None:
            raise _lib.MiError('libmi_maml error -1: lr_vec is None: meta_batch_anil_lr takes the step sizes of the head on the device')
        return self._anil_call(theta, data, labels, shots, adapt_steps, None, lr_vec, None, first_order, with_grad, want_lr_grad, return_logits)

    @_on_device
    def meta_batch_anil_steps(self, theta, data, labels, shots, adapt_steps, step_w, inner_lr=None, lr_vec=None, first_order=False, with_grad=True,
                              want_lr_grad=False, return_logits=False):
        """`meta_batch_anil` / `meta_batch_anil_lr` with the query set scored after 0, 1, .., adapt_steps head steps in the one call (the
        trunk still runs once), and the multi-step loss sum_j step_w[j - 1] * L_query(theta_j) as the outer objective
        (mi_meta_batch_anil_steps).  step_w [adapt_steps] fp32 on the engine's device, read there by every call, graph replays included.
        Exactly one of inner_lr (a number) and lr_vec (as in `meta_batch_anil_lr`).
        Returns (loss [K + 1, T], acc [K + 1, T], meta_grad [P] or None, lr_grad or None, logits [K + 1, T, S*W, ways] or None)."""
        if (inner_lr is None) == (lr_vec is None):
            raise ValueError('meta_batch_anil_steps takes exactly one of inner_lr and lr_vec')
        if step_w is None:
            raise _lib.MiError('libmi_maml error -1: step_w is None: meta_batch_anil_steps takes adapt_steps weights on the device')
        return self._anil_call(theta, data, labels, shots, adapt_steps, inner_lr, lr_vec, step_w, first_order, with_grad, want_lr_grad,
                               return_logits)

    @_on_device
    def meta_batch_anil_proto(self, theta, data, labels, shots, adapt_steps, scale, inner_lr=None, lr_vec=None, step_w=None, first_order=False,
                              with_grad=True, want_lr_grad=False, return_logits=False):
        """Proto-MAML on the ANIL trunk (mi_meta_batch_anil_proto): `meta_batch_anil_lr` / `meta_batch_anil_steps` with the head's
        initialisation derived per task from the support prototypes, W_0[w] = 2 scale c_w, b_0[w] = -scale |c_w|^2, and differentiated
        through.  adapt_steps = 0 (without step_w) is Prototypical Networks; with step_w, row 0 of the outputs is its score.  The head's
        entries of theta are not used and their gradient is exactly zero.  Exactly one of inner_lr and lr_vec (adapt_steps = 0: neither is
        fine).  Returns (loss, acc, meta_grad[P] or None, lr_grad or None, dscale [T] or None, logits or None), loss / acc / logits with a
        leading axis of adapt_steps + 1 when step_w is given; dscale[t] = d objective_t / d scale, per task: the sum is the caller's."""
        scale = float(scale)
        if not (scale > 0.0 and math.isfinite(scale)):
            raise _lib.MiError(f'libmi_maml error -1: the prototype initialisation\'s scale must be positive and finite, got {scale}')
        if inner_lr is not None and lr_vec is not None or (inner_lr is None and lr_vec is None and int(adapt_steps) > 0):
            raise ValueError('meta_batch_anil_proto takes exactly one of inner_lr and lr_vec')
        return self._anil_call(theta, data, labels, shots, adapt_steps, 0.0 if inner_lr is None else inner_lr, lr_vec, step_w, first_order,
                               with_grad, want_lr_grad, return_logits, proto_scale=scale)

    @_on_device
    def proto_init(self, fs, ys, ways, scale):
        """The prototype initialisation's kernel entry (mi_proto_init) on given support features: fs [T, ns, F] fp32, ys [T, ns] int32 in
        [0, ways), every class with at least one support row.  Returns [T, ways * F + ways]: per task W_0 [ways, F], then b_0 [ways]."""
        T, ns, feat = self._proto_check(fs, ys)
        head = torch.empty(T, int(ways) * feat + int(ways), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_proto_init(_stream(self.device), _ptr(fs), _ptr(ys), T, ns, feat, int(ways), float(scale), _ptr(head), head.shape[1]), None)
        return head

    @_on_device
    def proto_init_bwd(self, fs, ys, lam_head, ways, scale, dfs=None, want_dscale=True):
        """mi_proto_init_bwd: lam_head [T, ways * F + ways] = d objective / d (W_0, b_0) as `proto_init` lays them out.  Adds the gradient
        through the initialisation INTO dfs [T, ns, F] (zeros when None) and returns (dfs, dscale [T] or None)."""
        T, ns, feat = self._proto_check(fs, ys)
        ph = int(ways) * feat + int(ways)
        if lam_head.dtype != torch.float32 or not lam_head.is_cuda or not lam_head.is_contiguous() or tuple(lam_head.shape) != (T, ph):
            raise ValueError(f'lam_head must be a contiguous fp32 CUDA tensor of shape {(T, ph)}, got {tuple(lam_head.shape)}')
        if dfs is None:
            dfs = torch.zeros_like(fs)
        elif dfs.dtype != torch.float32 or not dfs.is_cuda or not dfs.is_contiguous() or dfs.shape != fs.shape:
            raise ValueError('dfs must be a contiguous fp32 CUDA tensor of fs\'s shape')
        dscale = torch.empty(T, dtype=torch.float32, device=self.device) if want_dscale else None
        _lib.check(self.lib.mi_proto_init_bwd(_stream(self.device), _ptr(fs), _ptr(ys), _ptr(lam_head), ph, T, ns, feat, int(ways), float(scale),
                                              _ptr(dfs), _ptr(dscale)), None)
        return dfs, dscale

    @staticmethod
    def _proto_check(fs, ys):
        if fs.dtype != torch.float32 or ys.dtype != torch.int32 or not (fs.is_cuda and ys.is_cuda) or not (fs.is_contiguous() and ys.is_contiguous()) \
                or fs.dim() != 3 or tuple(ys.shape) != tuple(fs.shape[:2]):
            raise ValueError(f'fs [T, ns, F] contiguous fp32 CUDA, ys [T, ns] contiguous int32 CUDA; got {tuple(fs.shape)}, {tuple(ys.shape)}')
        return tuple(fs.shape)

    def _closed_form_call(self, name, key, theta, data, labels, shots, hyper, with_grad, return_logits, n_hyper=0):
        """mi_meta_batch_<name>, the fused call of a closed-form head with the hyper-parameters `hyper`.  `key`: the outputs' persistent set in
        graph mode, distinct per head (and per metric).  n_hyper > 0: a call with a gradient also gives the per-task hyper-parameter
        gradients [T, n_hyper], between meta_grad and logits in the arguments and in the result."""
        s = self.spec
        T = self._check_batch(theta, data, labels, shots, flat_data=False)
        b = C.c_size_t()
        _lib.check(getattr(self.lib, f'mi_{name}_workspace_bytes')(self._h, T, s.ways, shots, int(bool(with_grad)), C.byref(b)), self._h)
        ws = self._workspace(b.value)
        loss, acc, grad, logits = self._outputs(key, T, shots * s.ways, with_grad, return_logits)
        dhyper = ()
        if n_hyper:
            dhyper = (self._persistent((f'{name}_dhyper', T), lambda: torch.empty(T, n_hyper, dtype=torch.float32, device=self.device))
                      if with_grad else None,)
        rc = self._fused_call(getattr(self.lib, f'mi_meta_batch_{name}'), _ptr(theta), _ptr(data), _ptr(labels), T, s.ways, shots, *hyper,
                              int(bool(with_grad)), _ptr(loss), _ptr(acc), _ptr(grad), *map(_ptr, dhyper), _ptr(logits), _ptr(ws), ws.numel())
        _lib.check(rc, self._h)
        return (loss, acc, grad) + dhyper + (logits,)

    def _head_entry(self, name, fs, fq, ys, yq, ways, hyper, with_grad, n_hyper=0):
        """mi_<name>_head, the kernel entry of a closed-form head on given features.  Returns (loss, acc, logits, dfs, dfq), and with
        n_hyper > 0 the per-task hyper-parameter gradients [T, n_hyper] as a sixth; the gradients are None without with_grad."""
        for t, dt in ((fs, torch.float32), (fq, torch.float32), (ys, torch.int32), (yq, torch.int32)):
            if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError('fs / fq must be contiguous fp32 CUDA tensors, ys / yq contiguous int32 CUDA tensors')
        if fs.dim() != 3 or fq.dim() != 3 or fs.shape[0] != fq.shape[0] or fs.shape[2] != fq.shape[2] or \
                tuple(ys.shape) != tuple(fs.shape[:2]) or tuple(yq.shape) != tuple(fq.shape[:2]):
            raise ValueError(f'fs [T, ns, F], fq [T, nq, F], ys [T, ns], yq [T, nq]; got {tuple(fs.shape)}, {tuple(fq.shape)}, '
                             f'{tuple(ys.shape)}, {tuple(yq.shape)}')
        T, ns, feat = fs.shape
        nq = fq.shape[1]
        loss = torch.empty(T, dtype=torch.float32, device=self.device)
        acc = torch.empty(T, dtype=torch.float32, device=self.device)
        logits = torch.empty(T, nq, ways, dtype=torch.float32, device=self.device)
        grads = (torch.empty_like(fs) if with_grad else None, torch.empty_like(fq) if with_grad else None)
        if n_hyper:
            grads += (torch.empty(T, n_hyper, dtype=torch.float32, device=self.device) if with_grad else None,)
        nscr = getattr(self.lib, f'mi_{name}_head_scratch_bytes')(T, ns, nq, feat, int(ways))
        scr = torch.empty(nscr, dtype=torch.uint8, device=self.device) if nscr else None
        _lib.check(getattr(self.lib, f'mi_{name}_head')(_stream(self.device), _ptr(fs), _ptr(fq), _ptr(ys), _ptr(yq), T, ns, nq, feat, int(ways),
                                                        *hyper, _ptr(loss), _ptr(acc), _ptr(logits), *map(_ptr, grads), _ptr(scr), nscr), None)
        return (loss, acc, logits) + grads

    @_on_device
    def meta_batch_metric(self, theta, data, labels, shots, metric='proto', scale=1.0, with_grad=True, return_logits=False):
        """A closed-form head on the ANIL trunk, no inner loop (mi_meta_batch_metric): metric 'proto' (Prototypical Networks: the class
        means, logits -scale * squared distance) or 'cosine' (NIL: logits scale * sum of the cosine similarities to a class's support
        rows).  theta keeps the ANIL layout [features.parameters()..., head.weight, head.bias]; the head's entries are not used and their
        gradient is exactly zero.  Returns (loss[T], acc[T], meta_grad[P] or None, logits [T, S*W, ways] or None)."""
        m, scale = metric_id(metric), check_scale(scale)
        return self._closed_form_call('metric', ('metric', m), theta, data, labels, shots, (m, scale), with_grad, return_logits)

    @_on_device
    def metric_head(self, fs, fq, ys, yq, ways, metric='proto', scale=1.0, with_grad=True):
        """The metric heads' kernel entry (mi_metric_head) on given features: fs [T, ns, F], fq [T, nq, F] fp32, ys [T, ns], yq [T, nq]
        int32 in [0, ways), every class with at least one support row.  Returns (loss[T], acc[T], logits [T, nq, ways], dfs, dfq), the
        last two None without a gradient."""
        m, scale = metric_id(metric), check_scale(scale)
        return self._head_entry('metric', fs, fq, ys, yq, ways, (m, scale), with_grad)

    @_on_device
    def meta_batch_ridge(self, theta, data, labels, shots, lam=1.0, scale=1.0, with_grad=True, return_logits=False):
        """The ridge-regression head (R2-D2) on the ANIL trunk (mi_meta_batch_ridge): per task A = (fs fs^T + lam I)^-1 onehot(ys), logits
        scale * (fq fs^T) A -- the head's inner problem solved exactly, no inner loop.  theta keeps the ANIL layout; the head's entries
        are not used and their gradient is exactly zero.  Returns (loss[T], acc[T], meta_grad[P] or None, dhyper [T, 2] or None, logits
        [T, S*W, ways] or None); dhyper[t] = (dloss_t/dlam, dloss_t/dscale), per task: the sum is the caller's."""
        return self._closed_form_call('ridge', ('ridge',), theta, data, labels, shots, check_ridge(lam, scale), with_grad, return_logits, n_hyper=2)

    @_on_device
    def ridge_head(self, fs, fq, ys, yq, ways, lam=1.0, scale=1.0, with_grad=True):
        """The ridge head's kernel entry (mi_ridge_head) on given features: fs [T, ns, F], fq [T, nq, F] fp32, ys [T, ns], yq [T, nq] int32
        in [0, ways).  Returns (loss[T], acc[T], logits [T, nq, ways], dfs, dfq, dhyper [T, 2]), the last three None without a gradient."""
        return self._head_entry('ridge', fs, fq, ys, yq, ways, check_ridge(lam, scale), with_grad, n_hyper=2)

    @_on_device
    def meta_batch_logreg(self, theta, data, labels, shots, lam=1.0, scale=1.0, with_grad=True, return_logits=False):
        """The logistic-regression head on the ANIL trunk (mi_meta_batch_logreg): per task the head's inner problem under softmax
        cross-entropy, W* = argmin sum_i CE(W fs_i, ys_i) + lam/2 |W|^2, solved to optimality and differentiated through the optimum; logits
        scale * fq W*^T.  theta keeps the ANIL layout; the head's entries are not used and their gradient is exactly zero.  Returns
        (loss[T], acc[T], meta_grad[P] or None, dhyper [T, 2] or None, logits [T, S*W, ways] or None); dhyper[t] = (dloss_t/dlam,
        dloss_t/dscale), per task: the sum is the caller's.  A task whose solve does not converge within the header's caps is NaN."""
        return self._closed_form_call('logreg', ('logreg',), theta, data, labels, shots, check_logreg(lam, scale), with_grad, return_logits, n_hyper=2)

    @_on_device
    def logreg_head(self, fs, fq, ys, yq, ways, lam=1.0, scale=1.0, with_grad=True):
        """The logistic-regression head's kernel entry (mi_logreg_head) on given features: fs [T, ns, F], fq [T, nq, F] fp32, ys [T, ns],
        yq [T, nq] int32 in [0, ways).  Returns (loss[T], acc[T], logits [T, nq, ways], dfs, dfq, dhyper [T, 2]), the last three None
        without a gradient."""
        return self._head_entry('logreg', fs, fq, ys, yq, ways, check_logreg(lam, scale), with_grad, n_hyper=2)

    @_on_device
    def forward_logits(self, theta, x):
        """Plain forward (no adaptation): x [T, n, C, H, W] -> logits [T, n, ways]; BatchNorm uses each batch's statistics."""
        T, n = x.shape[0], x.shape[1]
        b = C.c_size_t()
        _lib.check(self.lib.mi_forward_workspace_bytes(self._h, T, n, C.byref(b)), self._h)
        ws = self._workspace(b.value)
        logits = torch.empty(T, n, self.spec.ways, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_forward_logits(self._h, _stream(self.device), _ptr(theta.contiguous()), _ptr(x.contiguous()), T, n,
                                              _ptr(logits), _ptr(ws), ws.numel()), self._h)
        return logits

    def _learner_args(self, theta, x):
        theta = theta.reshape(-1, self.param_count) if theta.dim() == 1 else theta
        if theta.dim() != 2 or theta.shape[1] != self.param_count or theta.shape[0] not in (1, x.shape[0]):
            raise ValueError(f'theta must be [P] or [1 | tasks, P] with P={self.param_count}, got {tuple(theta.shape)}')
        for t in (theta, x):
            if t.dtype != torch.float32 or not t.is_cuda:
                raise ValueError('theta / x must be fp32 CUDA tensors')
        if x.dim() != 5 or tuple(x.shape[2:]) != (self.spec.in_channels, self.spec.in_h, self.spec.in_w):
            raise ValueError(f'x must be [tasks, n, {self.spec.in_channels}, {self.spec.in_h}, {self.spec.in_w}], got {tuple(x.shape)}')
        T, n = x.shape[0], x.shape[1]
        b = C.c_size_t()
        _lib.check(self.lib.mi_forward_workspace_bytes(self._h, T, n, C.byref(b)), self._h)
        return theta.contiguous(), x.contiguous(), T, n, self._workspace(b.value)

    @_on_device
    def learner_forward(self, theta, x, rep_layer=None, want_logits=True):
        """`learner(x)` with caller-held fast weights: theta [P] / [1,P] (shared) or [T,P]; x [T, n, C, H, W].
        Returns (logits [T,n,ways] or None, rep or None) where rep = output of the first `rep_layer` ConvBlocks in NCHW
        (reference get_rep_layer, vision_models.py:60-63,115-118)."""
        theta, x, T, n, ws = self._learner_args(theta, x)
        logits = torch.empty(T, n, self.spec.ways, dtype=torch.float32, device=self.device) if want_logits else None
        rep = None
        if rep_layer is not None:
            c, h, w = self.spec.block_output_shape(rep_layer)
            rep = torch.empty(T, n, c, h, w, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_learner_forward(self._h, _stream(self.device), _ptr(theta), theta.shape[0], _ptr(x), T, n, _ptr(logits),
                                               int(rep_layer or 0), _ptr(rep), _ptr(ws), ws.numel()), self._h)
        return logits, rep

    @_on_device
    def learner_backward(self, theta, x, dlogits):
        """Vector-Jacobian product of `learner(x)`: d sum(logits*dlogits)/d theta, [theta_tasks, P] (first derivatives)."""
        theta, x, T, n, ws = self._learner_args(theta, x)
        dlogits = dlogits.to(torch.float32).contiguous()
        if tuple(dlogits.shape) != (T, n, self.spec.ways):
            raise ValueError(f'dlogits must be {(T, n, self.spec.ways)}, got {tuple(dlogits.shape)}')
        grad = torch.empty(theta.shape[0], self.param_count, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_learner_backward(self._h, _stream(self.device), _ptr(theta), theta.shape[0], _ptr(x), _ptr(dlogits), T, n,
                                                _ptr(grad), _ptr(ws), ws.numel()), self._h)
        return grad

    @_on_device
    def learner_hvp(self, theta, x, dlogits, v):
        """mi_learner_hvp: the vector-Jacobian products of (theta, dlogits) -> learner_backward(theta, x, dlogits) for a cotangent v
        [theta_tasks, P] on that gradient: ((d^2 sum(logits*dlogits)/dtheta^2) v  [theta_tasks, P],  J(theta) v  [T, n, ways])."""
        theta, x, T, n, _ = self._learner_args(theta, x)
        dlogits = dlogits.to(torch.float32).contiguous()
        v = v.to(torch.float32).reshape(theta.shape).contiguous()
        if tuple(dlogits.shape) != (T, n, self.spec.ways):
            raise ValueError(f'dlogits must be {(T, n, self.spec.ways)}, got {tuple(dlogits.shape)}')
        b = C.c_size_t()
        _lib.check(self.lib.mi_learner_hvp_workspace_bytes(self._h, T, n, C.byref(b)), self._h)
        ws = self._workspace(b.value)
        gtheta = torch.empty(theta.shape[0], self.param_count, dtype=torch.float32, device=self.device)
        ldot = torch.empty(T, n, self.spec.ways, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_learner_hvp(self._h, _stream(self.device), _ptr(theta), theta.shape[0], _ptr(x), _ptr(dlogits), _ptr(v), T, n,
                                           _ptr(gtheta), _ptr(ldot), _ptr(ws), ws.numel()), self._h)
        return gtheta, ldot

    @_on_device
    def head_logits(self, f, wl, bl):
        """`linear(f)` for f [n, F] with explicit weights (reference get_rep_layer(x, -1)); mi_head_fwd_bwd, forward only."""
        f, wl, bl = f.contiguous(), wl.contiguous().float(), bl.contiguous().float()
        n, feat, ways = f.shape[0], f.shape[1], wl.shape[0]
        y = torch.zeros(n, dtype=torch.int32, device=self.device)
        scr = torch.empty(max(2 * n, n * feat), dtype=torch.float32, device=self.device)
        la = torch.empty(2, dtype=torch.float32, device=self.device)
        logits = torch.empty(n, ways, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.mi_head_fwd_bwd(_stream(self.device), _ptr(f), _ptr(wl), _ptr(bl), 0, _ptr(y), 1, n, feat, ways, _ptr(la[:1]),
                                            _ptr(la[1:]), _ptr(logits), None, None, None, None, 0, _ptr(scr)), self._h)
        return logits

    def profile(self, on, op=None, layer=0):
        """Record HIP events around every launch (or only launches of one (op name, layer)) until switched off."""
        kind = -1
        if op is not None:
            names = [self.lib.mi_profile_op_name(i).decode() for i in range(self.lib.mi_profile_kinds() // 8)]
            kind = names.index(op) * 8 + layer
        _lib.check(self.lib.mi_profile_enable(self._h, int(on), kind), self._h)

    def profile_collect(self):
        """{(op name, layer): (total_ms, launches)} since the last collect; synchronises on the recorded events."""
        n = self.lib.mi_profile_kinds()
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        _lib.check(self.lib.mi_profile_collect(self._h, ms, cnt, n), self._h)
        return {(self.lib.mi_profile_op_name(k // 8).decode(), k % 8): (ms[k], cnt[k]) for k in range(n) if cnt[k]}

    @_on_device
    def adam_step(self, theta, grad, state, lr, grad_scale=1.0, betas=(0.9, 0.999), eps=1e-8):
        """torch.optim.Adam defaults on the flat meta-parameters (vision/maml_vision.py:85,139-141)."""
        if 'm' not in state:
            state['m'] = torch.zeros_like(theta)
            state['v'] = torch.zeros_like(theta)
            state['step'] = 0
        state['step'] += 1
        _lib.check(self.lib.mi_adam_step(_stream(self.device), _ptr(theta), _ptr(grad), _ptr(state['m']), _ptr(state['v']),
                                         theta.numel(), state['step'], lr, betas[0], betas[1], eps, grad_scale))


def gae_max_rows(state_dim):
    """Longest replay mi_gae_advantages takes for this state dimension (0: unsupported dimension)."""
    return int(_lib.load().mi_gae_max_rows(int(state_dim)))


def gae_advantages(states, next_states, rewards, dones, count, gamma, tau, reg, normalize=True, want_weights=False, weights=None):
    """mi_gae_advantages: cherry-semantics returns -> LinearValue fit -> bootstraps -> GAE (-> ch.normalize) for R replays in one
    launch (reference core_functions/rl.py:95-110,355).  states / next_states [R, B, S], rewards / dones [R, B] fp32 CUDA tensors,
    count [R] int32 (rows in use) or None; weights [R, 2S+4] fp64: use these baseline weights instead of fitting (update_vf=False).
    Returns adv [R, B] fp32 (and the baseline weights [R, 2S+4] fp64)."""
    lib = _lib.load()
    dev = states.device
    R, B, S = states.shape
    f32 = lambda t, shape: t.to(dev, torch.float32).reshape(shape).contiguous()
    states, next_states = f32(states, (R, B, S)), f32(next_states, (R, B, S))
    rewards, dones = f32(rewards, (R, B)), f32(dones, (R, B))
    if count is not None:
        count = count.to(dev, torch.int32).contiguous()
    adv = torch.empty(R, B, dtype=torch.float32, device=dev)
    wts = torch.empty(R, 2 * S + 4, dtype=torch.float64, device=dev) if want_weights else None
    if weights is not None:
        weights = weights.to(dev, torch.float64).reshape(R, 2 * S + 4).contiguous()
    with torch.cuda.device(dev):
        _lib.check(lib.mi_gae_advantages(_stream(dev), _ptr(states), _ptr(next_states), _ptr(rewards), _ptr(dones), _ptr(count), _ptr(weights), R, B, S,
                                         float(gamma), float(tau), float(reg), int(bool(normalize)), _ptr(adv), _ptr(wts)))
    return (adv, wts) if want_weights else adv


def copy_segments(src_ptrs, dst_ptrs, nfloat, npad, dev):
    """mi_copy_segments: segment k = nfloat[k] floats from device address src_ptrs[k] to dst_ptrs[k], zeros up to npad[k] floats (lists of
    ints).  The caller keeps the tensors alive and has checked them (fp32, contiguous, on ``dev``)."""
    n = len(src_ptrs)
    if n == 0:
        return
    vp, u32 = C.c_void_p * n, C.c_uint32 * n
    with torch.cuda.device(dev):
        _lib.check(_lib.load().mi_copy_segments(_stream(dev), vp(*src_ptrs), vp(*dst_ptrs), u32(*nfloat), u32(*npad), n))


def upload_int32(values, dev):
    """A short list of ints as an int32 device tensor through mi_upload_i32: the values travel in kernel arguments (a pageable
    host-to-device copy of a few bytes blocks the host for ~50 us on this stack)."""
    n = len(values)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.load().mi_upload_i32(_stream(dev), _ptr(out), (C.c_int32 * n)(*values), n))
    return out


def _as_i32(u):
    """An unsigned 32-bit value as the int32 with the same bits."""
    return u - (1 << 32) if u >= (1 << 31) else u


def flatten_parameters(module):
    """Flat fp32 vector in module.parameters() order (what the C ABI calls theta)."""
    return torch.cat([p.detach().reshape(-1) for p in module.parameters()]).float().contiguous()


class PolicyEngine:
    """ctypes wrapper of the MAML-TRPO policy path (mi_policy_* / mi_trpo_*), batched over tasks."""

    def __init__(self, state_size, action_size, hiddens=(100, 100), device=None, activation='relu'):
        self.lib = _lib.load()
        if activation not in ('relu', 'tanh'):
            raise NotImplementedError(f'activation {activation!r}: the reference offers relu and tanh (policies.py:32-37)')
        if not torch.cuda.is_available():
            raise _lib.MiError('PolicyEngine needs a GPU: there is no CPU implementation of the policy path in this package.')
        if len(hiddens) != 2:
            raise ValueError('the HIP policy path implements the reference default: two hidden layers (policies.py:33-34)')
        self.device = _resolve_device(device)
        self.S, self.A, self.H = state_size, action_size, tuple(hiddens)
        desc = _lib.MiPolicyDesc(state_size, action_size, hiddens[0], hiddens[1], int(activation == 'tanh'))
        self._h = C.c_void_p()
        rc = self.lib.mi_policy_create(C.byref(desc), self.device.index, C.byref(self._h))
        if rc:
            raise _lib.MiError(self.lib.mi_policy_last_error(None).decode())
        n = C.c_size_t()
        self.lib.mi_policy_param_count(self._h, C.byref(n))
        self.param_count = n.value
        self._ws = None

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and h.value:
            self.lib.mi_policy_destroy(h)
            self._h = C.c_void_p()

    def _check(self, rc):
        if rc:
            raise _lib.MiError(f'libmi_maml policy error {rc}: {self.lib.mi_policy_last_error(self._h).decode()}')

    def _workspace(self, T, B, K=1, lr_rows=0):
        # the ANIL-TRPO plan of K updates starts with the MAML-TRPO one (which forward and adapt fit into): one buffer serves all,
        # and a kl_prepare after surrogate finds the surrogate's per-update passes where it left them.  lr_rows: the step-size-vector
        # calls, whose plan is the same one with one more array behind it
        b = C.c_size_t()
        if lr_rows:
            self._check(self.lib.mi_trpo_general_steps_lr_workspace_bytes(self._h, T, B, K, lr_rows, C.byref(b)))
        else:
            self._check(self.lib.mi_trpo_general_steps_workspace_bytes(self._h, T, B, K, C.byref(b)))
        return self._grow_workspace(b.value)

    def _grow_workspace(self, nbytes):
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    @_on_device
    def forward(self, theta, states):
        """loc of the policy density; theta [P] (shared) or [T, P]; states [T, B, S] -> loc [T, B, A]."""
        T, B = states.shape[0], states.shape[1]
        ws = self._workspace(T, B)
        loc = torch.empty(T, B, self.A, device=self.device)
        stride = 0 if theta.dim() == 1 else self.param_count
        self._check(self.lib.mi_policy_forward(self._h, _stream(self.device), _ptr(theta.contiguous()), stride, _ptr(states.contiguous()), T, B,
                                               _ptr(loc), _ptr(ws), ws.numel()))
        return loc

    @_on_device
    def rollout(self, theta, goals, rollout_ids, seed, episodes, max_path_length, want_noise=False):
        """mi_particles_rollout: ``episodes`` Particles2D episodes of up to ``max_path_length`` steps for every task, two launches in
        all and no synchronisation.  theta [P] (shared) or [T, P]; goals [T, 2] (tensor or array); rollout_ids: T integers in
        [0, 2^64) or an int64 device tensor holding their bit patterns; the noise is a pure function of (seed, id, episode, step).
        Returns the padded batch {states, actions, next_states [T, B, 2], rewards, dones [T, B], count [T] int32, ep_len [T, E]
        int32} with B = episodes * max_path_length, rows past count zero (+ noise [T, B, 2] with ``want_noise``)."""
        dev, f32 = self.device, torch.float32
        if torch.is_tensor(goals):
            goals = goals.detach().to(dev, f32).reshape(-1, 2).contiguous()
        else:
            import numpy as np
            g = np.ascontiguousarray(goals, dtype=np.float32).reshape(-1, 2)
            goals = upload_int32(g.view(np.int32).reshape(-1).tolist(), dev).view(f32).view(-1, 2)
        T, E, L = goals.shape[0], int(episodes), int(max_path_length)
        if torch.is_tensor(rollout_ids):
            ids = rollout_ids.to(dev, torch.int64).reshape(-1).contiguous()
        else:                                                  # the 64-bit ids as pairs of 32-bit halves, carried in kernel arguments
            halves = []
            for r in rollout_ids:
                r = int(r) & (2 ** 64 - 1)
                halves += [_as_i32(r & 0xffffffff), _as_i32(r >> 32)]
            ids = upload_int32(halves, dev).view(torch.int64)
        if ids.numel() != T:
            raise ValueError(f'{ids.numel()} rollout ids for {T} goals')
        theta = theta.detach()
        if theta.dtype != f32 or not theta.is_cuda or theta.dim() not in (1, 2) or theta.shape[-1] != self.param_count or \
                (theta.dim() == 2 and theta.shape[0] != T):
            raise ValueError(f'theta must be fp32 on the GPU, [P] or [{T}, P] with P={self.param_count}, got {tuple(theta.shape)}')
        theta = theta.contiguous()
        stride = 0 if theta.dim() == 1 else self.param_count
        nb = int(self.lib.mi_particles_rollout_scratch_bytes(self._h, T, E, L))
        ws = getattr(self, '_rollout_ws', None)
        if nb and (ws is None or ws.numel() < nb):
            ws = self._rollout_ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        B = max(E * L, 0)
        out = dict(states=torch.empty(T, B, 2, dtype=f32, device=dev), actions=torch.empty(T, B, 2, dtype=f32, device=dev),
                   next_states=torch.empty(T, B, 2, dtype=f32, device=dev), rewards=torch.empty(T, B, dtype=f32, device=dev),
                   dones=torch.empty(T, B, dtype=f32, device=dev), count=torch.empty(T, dtype=torch.int32, device=dev),
                   ep_len=torch.empty(T, max(E, 0), dtype=torch.int32, device=dev))
        if want_noise:
            out['noise'] = torch.empty(T, B, 2, dtype=f32, device=dev)
        self._check(self.lib.mi_particles_rollout(
            self._h, _stream(dev), _ptr(theta), stride, _ptr(goals), _ptr(ids), int(seed) & (2 ** 64 - 1), T, E, L, _ptr(out['states']),
            _ptr(out['actions']), _ptr(out['next_states']), _ptr(out['rewards']), _ptr(out['dones']), _ptr(out['count']),
            _ptr(out['ep_len']), _ptr(out.get('noise')), _ptr(ws), ws.numel() if ws is not None else 0))
        return out

    def _lr_table(self, lr, K, step_lr_row, one_row=False, row0_default=False):
        """THE check of a call's step: None for a number (the scalar entries), else (lr_vec [rows, P] fp32 contiguous on the device, rows,
        the int32 array of the K updates' rows or None = row 0 for all) for a [rows, P] / [P] tensor in the engine's parameter order.
        one_row: adapt / update take [P] only.  row0_default: the meta-batch reads row 0 of any table where no rows are named."""
        if not torch.is_tensor(lr):
            if step_lr_row is not None:
                raise ValueError('step_lr_row goes with a step-size tensor, not with a number')
            return None
        P = self.param_count
        lr = lr.detach()
        if one_row and lr.dim() != 1:
            raise ValueError(f'lr must be a number or ONE row [P] of step sizes, got {tuple(lr.shape)}')
        if lr.dim() == 1:
            lr = lr.unsqueeze(0)
        if lr.dim() != 2 or lr.shape[1] != P or lr.shape[0] < 1 or lr.dtype != torch.float32 or not lr.is_cuda:
            raise ValueError(f'the step must be a number or an fp32 tensor on the GPU, [rows, P] or [P] with P={P}, got {tuple(lr.shape)} {lr.dtype}')
        rows = lr.shape[0]
        if step_lr_row is None:
            if rows != 1 and not row0_default:
                raise ValueError(f'a step-size table of {rows} rows needs step_lr_row (the row each of the {K} updates reads)')
            return lr.contiguous(), rows, None
        if len(step_lr_row) != K:
            raise ValueError(f'step_lr_row holds {len(step_lr_row)} rows for {K} updates')
        return lr.contiguous(), rows, (C.c_int32 * max(K, 1))(*[int(x) for x in step_lr_row])

    def _step_args(self, lr, K, step_lr_row, one_row=False):
        """The header's rule for the step-size-table entries ("its scalar namesake with lr_vec, lr_rows, step_lr_row where that takes
        float inner_lr"; adapt / update, ``one_row``: lr_vec alone) -> (the suffix of the entry's symbol, the arguments that stand
        there, the table's rows or 0, the table itself: it must outlive the call)."""
        tab = self._lr_table(lr, K, step_lr_row, one_row)
        if tab is None:
            return '', (float(lr),), 0, None
        vec, rows, sr = tab
        return '_lr', ((_ptr(vec),) if one_row else (_ptr(vec), rows, sr)), rows, vec

    @_on_device
    def adapt(self, theta, states, actions, adv, count, lr, head_only=False):
        """trpo_update for T tasks: returns (theta_out [T, P], loss [T]).  head_only: ANIL inner loop (body under no_grad).  ``lr``: a
        number, or a [P] fp32 tensor of per-parameter step sizes in the engine's order (mi_policy_adapt_lr; an entry whose step is 0
        keeps the bits of theta)."""
        T, B = states.shape[0], states.shape[1]
        ws = self._workspace(T, B)
        out = torch.empty(T, self.param_count, device=self.device)
        loss = torch.empty(T, device=self.device)
        stride = 0 if theta.dim() == 1 else self.param_count
        sfx, step, _, _keep = self._step_args(lr, 1, None, one_row=True)
        self._check(getattr(self.lib, 'mi_policy_adapt' + sfx)(
            self._h, _stream(self.device), _ptr(theta.contiguous()), stride, _ptr(states), _ptr(actions), _ptr(adv), _ptr(count), T, B, *step,
            int(head_only), _ptr(out), _ptr(loss), _ptr(ws), ws.numel()))
        return out, loss

    def _trpo_shapes(self, sup, qry, theta=None, old_loc=None, old_scale=None, v=None):
        """(K, T, B) of a TRPO call, every array checked against them: the library sizes all its reads from these three numbers, so a
        support replay without its leading [K] axis -- or any other mismatch -- would be read out of bounds on the device."""
        shp = tuple(sup['states'].shape)
        if len(shp) != 4 or shp[3] != self.S:
            raise ValueError(f"sup['states'] must be [K, T, B, {self.S}] (the leading [K] axis also at K = 1), got {shp}")
        K, T, B = shp[:3]
        P, A = self.param_count, self.A
        want = [("sup['actions']", sup['actions'], (K, T, B, A)), ("sup['count']", sup['count'], (K, T)),
                ("qry['states']", qry['states'], (T, B, self.S)), ("qry['count']", qry['count'], (T,))]
        if theta is not None:       # surrogate: the advantages and the query actions are read as well
            want += [("sup['adv']", sup['adv'], (K, T, B)), ("qry['actions']", qry['actions'], (T, B, A)), ("qry['adv']", qry['adv'], (T, B)),
                     ('theta', theta, (P,))]
        want += [(n, x, s) for n, x, s in (('old_loc', old_loc, (T, B, A)), ('old_scale', old_scale, (T, A)), ('v', v, (P,))) if x is not None]
        for name, x, s in want:
            if tuple(x.shape) != s:
                raise ValueError(f'{name} must be {list(s)} for K, T, B = {K}, {T}, {B}, got {list(x.shape)}')
        return K, T, B

    @_on_device
    def surrogate(self, theta, sup, qry, old_loc, old_scale, inner_lr, want_grad, step_lr_row=None):
        """meta_surrogate_loss with K = sup['states'].shape[0] inner updates.  sup: dict with states [K,T,B,S], actions [K,T,B,A],
        adv [K,T,B], count [K,T] int32 (the leading [K] axis also at K = 1); qry: the same without it.  -> (loss, kl, grad or None).
        ``inner_lr``: a number, or (here and in ``fvp`` / ``kl_prepare`` / ``fvp_general``, which must be given the same) a [rows, P] / [P]
        fp32 tensor of fixed per-parameter step sizes in the engine's order, update k reading row ``step_lr_row[k]`` (None: one row)."""
        K, T, B = self._trpo_shapes(sup, qry, theta=theta, old_loc=old_loc, old_scale=old_scale)
        sfx, step, rows, _keep = self._step_args(inner_lr, K, step_lr_row)
        ws = self._workspace(T, B, K, rows)
        loss = torch.empty(1, device=self.device)
        kl = torch.empty(1, device=self.device)
        grad = torch.empty(self.param_count, device=self.device) if want_grad else None
        self._check(getattr(self.lib, 'mi_trpo_surrogate_steps' + sfx)(
            self._h, _stream(self.device), _ptr(theta), K, _ptr(sup['states']), _ptr(sup['actions']), _ptr(sup['adv']), _ptr(sup['count']),
            _ptr(qry['states']), _ptr(qry['actions']), _ptr(qry['adv']), _ptr(qry['count']), _ptr(old_loc), _ptr(old_scale), T, B,
            *step, _ptr(loss), _ptr(kl), _ptr(grad), _ptr(ws), ws.numel()))
        return loss, kl, grad

    @_on_device
    def fvp(self, sup, qry, inner_lr, damping, v, step_lr_row=None):
        """Fisher-vector product at the theta of the preceding ``surrogate`` call (same replays, same step)."""
        K, T, B = self._trpo_shapes(sup, qry, v=v)
        sfx, step, rows, _keep = self._step_args(inner_lr, K, step_lr_row)
        ws = self._workspace(T, B, K, rows)
        out = torch.empty(self.param_count, device=self.device)
        self._check(getattr(self.lib, 'mi_trpo_fvp_steps' + sfx)(
            self._h, _stream(self.device), K, _ptr(sup['states']), _ptr(sup['actions']), _ptr(sup['count']), _ptr(qry['states']),
            _ptr(qry['count']), T, B, *step, float(damping), _ptr(v.contiguous()), _ptr(out), _ptr(ws), ws.numel()))
        return out

    @_on_device
    def kl_prepare(self, sup, qry, old_loc, old_scale, inner_lr, want_grad=False, step_lr_row=None):
        """After ``surrogate`` at the same theta and replays: the context of the exact KL Hessian-vector product for
        new != old with K = sup['states'].shape[0] inner updates (ANIL-TRPO).  Returns d mean KL / d theta [P] if ``want_grad``."""
        K, T, B = self._trpo_shapes(sup, qry, old_loc=old_loc, old_scale=old_scale)
        sfx, step, rows, _keep = self._step_args(inner_lr, K, step_lr_row)
        ws = self._workspace(T, B, K, rows)
        grad = torch.empty(self.param_count, device=self.device) if want_grad else None
        self._check(getattr(self.lib, 'mi_trpo_kl_prepare_steps' + sfx)(
            self._h, _stream(self.device), K, _ptr(sup['states']), _ptr(sup['actions']), _ptr(sup['count']), _ptr(qry['states']),
            _ptr(qry['count']), _ptr(old_loc), _ptr(old_scale), T, B, *step, _ptr(grad), _ptr(ws), ws.numel()))
        return grad

    @_on_device
    def fvp_general(self, sup, qry, old_scale, inner_lr, damping, v, step_lr_row=None):
        """Exact Hessian-vector product of the mean KL at the theta of the preceding ``surrogate`` + ``kl_prepare``."""
        K, T, B = self._trpo_shapes(sup, qry, old_scale=old_scale, v=v)
        sfx, step, rows, _keep = self._step_args(inner_lr, K, step_lr_row)
        ws = self._workspace(T, B, K, rows)
        out = torch.empty(self.param_count, device=self.device)
        self._check(getattr(self.lib, 'mi_trpo_fvp_general_steps' + sfx)(
            self._h, _stream(self.device), K, _ptr(sup['states']), _ptr(sup['actions']), _ptr(sup['count']), _ptr(qry['states']),
            _ptr(qry['count']), _ptr(old_scale), T, B, *step, float(damping), _ptr(v.contiguous()), _ptr(out), _ptr(ws), ws.numel()))
        return out

    @_on_device
    def meta_batch(self, theta, sup, qry, step_batch, inner_lr, loss='a2c', clip=0.1, step_new_old=None, head_only=False,
                   first_order=False, with_grad=True):
        """K = len(step_batch) MAML updates of the policy on replayed support batches + validation loss + meta-gradient for all
        tasks (mi_policy_meta_batch: fast_adapt_vpg / fast_adapt_ppo, reference rl.py:231-255,267-318).
        sup: dict states [NB,T,B,S], actions [NB,T,B,A], adv [NB,T,B], count [NB,T] int32 (NB support batches); qry: the same
        without the NB axis.  Returns (loss [T], theta_adapted [T,P], grad [P] summed over tasks or None)."""
        return self._meta_call(theta, sup, qry, step_batch, float(inner_lr), None, loss, clip, step_new_old, head_only, first_order, with_grad,
                               False)[:3]

    def _meta_call(self, theta, sup, qry, step_batch, lr, step_lr_row, loss, clip, step_new_old, head_only, first_order, with_grad, want_lr_grad):
        """``meta_batch`` (``lr`` a number: mi_policy_meta_batch_dones, whose flags only the DiCE objective reads) and ``meta_batch_lr``
        (a tensor: mi_policy_meta_batch_lr) -> (loss, theta_adapted, grad or None, lr_grad or None)."""
        K = len(step_batch)
        T, B, P = qry['states'].shape[0], qry['states'].shape[1], self.param_count
        NB = sup['states'].shape[0] if K else 0
        kind = {'a2c': 0, 'ppo': 1, 'dice': 2}[loss]
        tab = self._lr_table(lr, K, step_lr_row, row0_default=True)
        want_lr_grad = bool(tab and want_lr_grad and with_grad)
        sb = (C.c_int32 * max(K, 1))(*[int(x) for x in step_batch])
        if step_new_old is None:
            step_new_old = [1 if (k == 0 or step_batch[k] != step_batch[k - 1]) else 0 for k in range(K)]
        sn = (C.c_int32 * max(K, 1))(*[int(x) for x in step_new_old])
        dice = loss == 'dice'    # the DiCE objective couples the samples of an episode: the replays' `dones` travel with them
        if dice and ('done' not in qry or (K and 'done' not in sup)):
            raise ValueError("loss='dice' needs the episode-end flags of every replay (key 'done', float32, like 'adv')")
        b, so = C.c_size_t(), int(not first_order and with_grad)
        if tab:
            self._check(self.lib.mi_policy_meta_lr_workspace_bytes(self._h, T, B, K, NB, so, tab[1], int(want_lr_grad), C.byref(b)))
        else:
            self._check(self.lib.mi_policy_meta_workspace_bytes(self._h, T, B, K, NB, so, C.byref(b)))
        ws = self._grow_workspace(b.value)
        loss_t = torch.empty(T, device=self.device)
        theta_out = torch.empty(T, P, device=self.device)
        grad = torch.empty(P, device=self.device) if with_grad else None
        lr_grad = torch.empty(tab[1], P, device=self.device) if want_lr_grad else None
        g = lambda d, k: _ptr(d[k].contiguous()) if d is not None and K else C.c_void_p(0)
        head = (self._h, _stream(self.device), _ptr(theta.contiguous()), K, sb, sn)
        replays = (NB, g(sup, 'states'), g(sup, 'actions'), g(sup, 'adv'), g(sup, 'count'), g(sup, 'done') if dice else None,
                   _ptr(qry['states'].contiguous()), _ptr(qry['actions'].contiguous()), _ptr(qry['adv'].contiguous()),
                   _ptr(qry['count'].contiguous()), _ptr(qry['done'].contiguous()) if dice else None, T, B, kind, float(clip))
        flags = (int(head_only), int(not first_order), int(with_grad), _ptr(loss_t), _ptr(theta_out), _ptr(grad))
        if tab:
            self._check(self.lib.mi_policy_meta_batch_lr(*head, tab[2], *replays, _ptr(tab[0]), tab[1], *flags, _ptr(lr_grad), _ptr(ws),
                                                         ws.numel()))
        else:
            self._check(self.lib.mi_policy_meta_batch_dones(*head, *replays, float(lr), *flags, _ptr(ws), ws.numel()))
        return loss_t, theta_out, grad, lr_grad

    @_on_device
    def meta_batch_lr(self, theta, sup, qry, step_batch, lr_vec, step_lr_row=None, loss='a2c', clip=0.1, step_new_old=None, head_only=False,
                      first_order=False, with_grad=True, want_lr_grad=True):
        """``meta_batch`` with per-parameter step sizes (mi_policy_meta_batch_lr): lr_vec [rows, P] (or [P]) fp32 in the engine's
        parameter order, update k reads row step_lr_row[k] (None: row 0).  Returns (loss [T], theta_adapted [T,P], grad [P] summed over
        tasks or None, lr_grad [rows, P] = d sum_t loss / d lr_vec or None).  ``want_lr_grad`` needs ``with_grad``; loss='dice' takes
        the replays' 'done' like ``meta_batch``."""
        if not torch.is_tensor(lr_vec):
            raise ValueError(f'lr_vec must be fp32 on the GPU, [rows, P] with P={self.param_count}, got {type(lr_vec).__name__}: meta_batch takes a number')
        return self._meta_call(theta, sup, qry, step_batch, lr_vec, step_lr_row, loss, clip, step_new_old, head_only, first_order, with_grad,
                               want_lr_grad)

    @_on_device
    def update(self, theta, states, actions, adv, count, lr, loss='a2c', epochs=1, clip=0.1, done=None, head_only=False):
        """mi_policy_update: ``epochs`` plain updates of every task's parameters on its own replay (the inner update of
        fast_adapt_vpg / fast_adapt_ppo, reference rl.py:231-255,267-318; single_ppo_update, rl.py:319-336).  theta [P] (shared) or
        [T, P]; states [T,B,S], actions [T,B,A], adv [T,B], count [T] int32 or None, done [T,B] (loss='dice').  PPO takes the old
        log-probabilities once, at the parameters the call starts from.  ``lr``: a number, or a [P] fp32 tensor of per-parameter step
        sizes in the engine's order (mi_policy_update_lr).  Returns (theta_out [T, P], loss [T, epochs]: the loss
        before each update).  No host synchronisation; the number of launches does not depend on T."""
        T, B = states.shape[0], states.shape[1]
        kind = {'a2c': 0, 'ppo': 1, 'dice': 2}[loss]
        if loss == 'dice' and done is None:
            raise ValueError("loss='dice' needs the episode-end flags of the replay (done [T, B], float32)")
        b = C.c_size_t()
        self._check(self.lib.mi_policy_update_workspace_bytes(self._h, T, B, C.byref(b)))
        ws = self._grow_workspace(b.value)
        theta = theta.detach()
        if theta.dim() == 2 and theta.shape[0] != T:
            raise ValueError(f'theta has {theta.shape[0]} rows for {T} tasks')
        out = torch.empty(T, self.param_count, device=self.device)
        losses = torch.empty(T, max(int(epochs), 1), device=self.device)
        stride = 0 if theta.dim() == 1 else self.param_count
        c = lambda t: None if t is None else t.contiguous()
        theta, states, actions, adv, count, done = c(theta), c(states), c(actions), c(adv), c(count), c(done)
        sfx, step, _, _keep = self._step_args(lr, 1, None, one_row=True)
        self._check(getattr(self.lib, 'mi_policy_update' + sfx)(
            self._h, _stream(self.device), _ptr(theta), stride, _ptr(states), _ptr(actions), _ptr(adv), _ptr(count), _ptr(done), T, B, kind,
            int(epochs), float(clip), *step, int(head_only), _ptr(out), _ptr(losses), _ptr(ws), ws.numel()))
        return out, losses

    # ------------------------------------------------------------------------------------------------- step-wise learner
    def _learner_workspace(self, T, B):
        """A buffer of its own: the TRPO context of ``surrogate`` / ``fvp`` lives in the other one between calls."""
        b = C.c_size_t()
        self._check(self.lib.mi_policy_learner_workspace_bytes(self._h, T, B, C.byref(b)))
        ws = getattr(self, '_learner_ws', None)
        if ws is None or ws.numel() < b.value:
            ws = self._learner_ws = torch.empty(b.value, dtype=torch.uint8, device=self.device)
        return ws

    def _learner_args(self, theta, states, dloc, count):
        f32 = torch.float32
        T, B = states.shape[0], states.shape[1]
        if theta.dim() not in (1, 2) or theta.shape[-1] != self.param_count or (theta.dim() == 2 and theta.shape[0] != T):
            raise ValueError(f'theta must be [P] or [{T}, P] with P={self.param_count}, got {tuple(theta.shape)}')
        if tuple(states.shape) != (T, B, self.S) or tuple(dloc.shape) != (T, B, self.A):
            raise ValueError(f'states [T, B, {self.S}] and dloc [T, B, {self.A}] expected, got {tuple(states.shape)} and {tuple(dloc.shape)}')
        conv = lambda x: x.detach().to(self.device, f32).contiguous()
        if count is not None:
            count = count.detach().to(self.device, torch.int32).contiguous()
            if count.numel() != T:
                raise ValueError(f'count holds {count.numel()} values for {T} tasks')
        return T, B, conv(theta), conv(states), conv(dloc), count, (0 if theta.dim() == 1 else self.param_count)

    @_on_device
    def vjp(self, theta, states, dloc, count=None, head_only=False):
        """mi_policy_vjp: grad [T, P] of s_t = sum_{row < count[t]} loc . dloc w.r.t. theta_t (sigma slots zero).  theta [P] (shared) or
        [T, P]; states [T, B, S]; dloc [T, B, A]; count [T] int32 or None.  head_only: only W3 / b3 receive a gradient."""
        T, B, theta, states, dloc, count, stride = self._learner_args(theta, states, dloc, count)
        ws = self._learner_workspace(T, B)
        grad = torch.empty(T, self.param_count, device=self.device)
        self._check(self.lib.mi_policy_vjp(self._h, _stream(self.device), _ptr(theta), stride, _ptr(states), _ptr(dloc), _ptr(count), T, B,
                                           int(bool(head_only)), _ptr(grad), _ptr(ws), ws.numel()))
        return grad

    @_on_device
    def hvp(self, theta, states, dloc, v, count=None, head_only=False):
        """mi_policy_hvp, the double backward of ``vjp`` for a direction v [T, P]: (hv [T, P] = (d^2 s_t / d theta^2) v_t with dloc held
        fixed, loc_dot [T, B, A] = J_t v_t, zero on rows past count)."""
        T, B, theta, states, dloc, count, stride = self._learner_args(theta, states, dloc, count)
        if tuple(v.shape) != (T, self.param_count):
            raise ValueError(f'v must be [{T}, {self.param_count}], got {tuple(v.shape)}')
        v = v.detach().to(self.device, torch.float32).contiguous()
        ws = self._learner_workspace(T, B)
        hv = torch.empty(T, self.param_count, device=self.device)
        loc_dot = torch.empty(T, B, self.A, device=self.device)
        self._check(self.lib.mi_policy_hvp(self._h, _stream(self.device), _ptr(theta), stride, _ptr(states), _ptr(dloc), _ptr(v), _ptr(count),
                                           T, B, int(bool(head_only)), _ptr(hv), _ptr(loc_dot), _ptr(ws), ws.numel()))
        return hv, loc_dot

    def learner_fused(self):
        """True if ``vjp`` / ``hvp`` of this shape take the fused sweep (while ``set_fused_learner`` is on)."""
        return bool(self.lib.mi_policy_learner_fused_supported(self._h))

    @staticmethod
    def set_fused_learner(on):
        """Process-wide ablation / test switch (default on): off runs ``vjp`` / ``hvp`` on the per-layer kernels at every shape."""
        _lib.load().mi_policy_set_fused_learner(int(bool(on)))
