"""``DiagNormalPolicy`` / ``DiagNormalPolicyANIL`` with the reference's constructors, parameter names/order and initialisers
(core_functions/policies.py:30-67,70-126); the MLP runs on the GPU through ``mi_policy_forward``.

Two call paths.  The bare policy (``policy.density(state)``, ``policy.log_prob(state, action)``, ``policy(state)``) is detached, as the
fused training calls use it.  With ``theta=`` (what a ``MAML`` wrapper passes: its fast weights, a flat vector in engine order) the mean
is a node of the autograd graph, differentiable to second order: first backward ``mi_policy_vjp``, second ``mi_policy_hvp``."""
import math

import torch
from torch import nn
from torch.distributions import Normal

from ..engine import PolicyEngine

EPSILON = 1e-6

_engines = {}


class _ThirdOrderGuard(torch.autograd.Function):
    """The results of mi_policy_hvp as functions of (theta, dloc, v) in the graph, with a backward that says what is missing."""

    @staticmethod
    def forward(ctx, theta, dloc, v, hv, loc_dot):
        return hv.view_as(hv), loc_dot.view_as(loc_dot)

    @staticmethod
    def backward(ctx, *gs):
        raise RuntimeError('the HIP policy differentiates to second order (mi_policy_vjp, mi_policy_hvp); a third derivative of '
                           'density / log_prob with respect to the parameters is not implemented')


class _PolicyLocVJP(torch.autograd.Function):
    """g = J(theta)^T dloc (mi_policy_vjp); its backward for a cotangent v on g is ONE mi_policy_hvp call:
    d(g.v)/dtheta = (d^2 s / dtheta^2) v and d(g.v)/ddloc = J v."""

    @staticmethod
    def forward(ctx, theta, dloc, states, engine, head_only):
        ctx.engine, ctx.head_only = engine, head_only
        ctx.save_for_backward(theta, dloc, states)
        return engine.vjp(theta.detach(), states, dloc.detach(), head_only=head_only)[0].to(theta.dtype)

    @staticmethod
    def backward(ctx, v):
        theta, dloc, states = ctx.saved_tensors
        hv, loc_dot = ctx.engine.hvp(theta.detach(), states, dloc.detach(), v.detach().reshape(1, -1), head_only=ctx.head_only)
        hv, loc_dot = hv[0].to(theta.dtype), loc_dot.to(dloc.dtype)
        if torch.is_grad_enabled():
            hv, loc_dot = _ThirdOrderGuard.apply(theta, dloc, v, hv, loc_dot)
        return hv, loc_dot, None, None, None


class _PolicyLoc(torch.autograd.Function):
    """loc [1, B, A] = MLP(theta; states [1, B, S]) (mi_policy_forward: the bits of the bare path).  States get no gradient."""

    @staticmethod
    def forward(ctx, theta, states, engine, head_only):
        ctx.engine, ctx.head_only = engine, head_only
        ctx.save_for_backward(theta, states)
        return engine.forward(theta.detach(), states)

    @staticmethod
    def backward(ctx, dloc):
        theta, states = ctx.saved_tensors
        return _PolicyLocVJP.apply(theta, dloc.contiguous(), states, ctx.engine, ctx.head_only), None, None, None


def linear_init(module):
    """reference policies.py:17-21"""
    if isinstance(module, nn.Linear):
        nn.init.xavier_uniform_(module.weight)
        module.bias.data.zero_()
    return module


class DiagNormalPolicy(nn.Module):
    def __init__(self, input_size, output_size, hiddens=None, activation='relu'):
        super().__init__()
        if hiddens is None:
            hiddens = [100, 100]
        if activation == 'relu':                                              # reference policies.py:32-37
            act = nn.ReLU
        elif activation == 'tanh':
            act = nn.Tanh
        else:
            raise NotImplementedError
        layers = [linear_init(nn.Linear(input_size, hiddens[0])), act()]
        for i, o in zip(hiddens[:-1], hiddens[1:]):
            layers += [linear_init(nn.Linear(i, o)), act()]
        layers.append(linear_init(nn.Linear(hiddens[-1], output_size)))
        self.sigma = nn.Parameter(torch.Tensor(output_size))                  # registered first (named_parameters order)
        self.sigma.data.fill_(math.log(1))
        self.mean = nn.Sequential(*layers)
        self.input_size, self.output_size, self.hiddens, self.activation = input_size, output_size, tuple(hiddens), activation

    def _engine_params(self):
        """Parameters in the engine's order: sigma, then (weight, bias) of the three Linear layers."""
        lin = [m for m in self.mean if isinstance(m, nn.Linear)]
        return [self.sigma] + [q for m in lin for q in (m.weight, m.bias)]

    def engine(self):
        dev = self.sigma.device
        if dev.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} computes only on the GPU (HIP engine); move it with .to("cuda")')
        key = (self.input_size, self.output_size, self.hiddens, self.activation, dev.index)
        if key not in _engines:
            _engines[key] = PolicyEngine(self.input_size, self.output_size, self.hiddens, dev, activation=self.activation)
        return _engines[key]

    def flat(self):
        """Flat parameter vector in the engine's order (sigma, W1, b1, W2, b2, W3, b3)."""
        return torch.cat([p.detach().reshape(-1) for p in self._engine_params()]).float().contiguous()

    def load_flat(self, theta):
        params = self._engine_params()
        f32 = torch.float32
        if (theta.is_cuda and theta.dtype is f32 and theta.is_contiguous() and
                all(p.is_cuda and p.dtype is f32 and p.is_contiguous() and p.get_device() == theta.get_device() for p in params)):
            # one mi_copy_segments launch scatters the vector into the parameter tensors (one copy launch per parameter otherwise)
            from ..engine import copy_segments
            base, srcs, cnts, off = theta.data_ptr(), [], [], 0
            for p in params:
                srcs.append(base + 4 * off)
                cnts.append(p.numel())
                off += p.numel()
            if off != theta.numel():
                raise ValueError(f'load_flat: {theta.numel()} values for {off} parameters')
            copy_segments(srcs, [p.data_ptr() for p in params], cnts, cnts, theta.device)      # (like a write through `.data`: no autograd version bump)
            return
        off = 0
        with torch.no_grad():
            for p in params:
                p.copy_(theta[off:off + p.numel()].view_as(p))
                off += p.numel()

    def flat_parameters(self):
        """The flat vector in the engine's order, CONNECTED to the parameters (what a ``MAML`` wrapper starts its fast weights from)."""
        return torch.cat([p.reshape(-1) for p in self._engine_params()])

    def density(self, state, theta=None):
        """reference policies.py:49-52.  ``theta`` None: the module's own parameters, detached.  ``theta`` [P] (engine order): loc
        through the differentiable HIP unit (``features_no_grad`` -> head_only: the body is a constant), scale = exp(clamp(sigma)) as
        plain torch ops on theta's sigma slots."""
        st = state.reshape(1, -1, self.input_size).float().contiguous()
        if theta is None:
            loc = self.engine().forward(self.flat(), st)[0].reshape(*state.shape[:-1], self.output_size)
            scale = torch.exp(torch.clamp(self.sigma.detach(), min=math.log(EPSILON)))
            return Normal(loc=loc, scale=scale)
        if theta.dim() != 1:
            raise ValueError(f'theta must be a flat parameter vector, got shape {tuple(theta.shape)}')
        loc = _PolicyLoc.apply(theta, st, self.engine(), bool(getattr(self, 'features_no_grad', False)))
        loc = loc[0].reshape(*state.shape[:-1], self.output_size)
        scale = torch.exp(torch.clamp(theta[:self.output_size], min=math.log(EPSILON)))
        return Normal(loc=loc, scale=scale)

    def log_prob(self, state, action, theta=None):
        """reference policies.py:54-56"""
        return self.density(state, theta).log_prob(action).mean(dim=1, keepdim=True)

    def forward(self, state, theta=None):
        """reference policies.py:58-61 (sampling never needs a graph)"""
        if theta is None:
            return self.density(state).sample()
        with torch.no_grad():
            return self.density(state, theta).sample()


class DiagNormalPolicyANIL(DiagNormalPolicy):
    """reference policies.py:70-126: tanh body (`self.body`), linear head (`self.head`), `sigma` registered last;
    `turn_off_body_grads()` puts the body under no_grad for the inner loop (rl.py:381-382), which on this engine is the
    `head_only` mode of mi_policy_adapt."""

    def __init__(self, input_size, output_size, fc_neurons, hiddens=None):
        nn.Module.__init__(self)
        if hiddens is None:
            hiddens = [100, 100]
        if len(hiddens) != 2 or fc_neurons != hiddens[-1]:
            raise ValueError('fc_neurons must equal the width of the last hidden layer (head = Linear(fc_neurons, output_size))')
        self.fc_neurons = fc_neurons
        layers = [linear_init(nn.Linear(input_size, hiddens[0])), nn.Tanh()]
        for i, o in zip(hiddens[:-1], hiddens[1:]):
            layers += [linear_init(nn.Linear(i, o)), nn.Tanh()]
        self.body = nn.Sequential(*layers)
        self.head = linear_init(nn.Linear(fc_neurons, output_size))
        self.sigma = nn.Parameter(torch.Tensor(output_size))
        self.sigma.data.fill_(math.log(1))
        self.features_no_grad = False
        self.input_size, self.output_size, self.hiddens, self.activation = input_size, output_size, tuple(hiddens), 'tanh'

    def _engine_params(self):
        lin = [m for m in self.body if isinstance(m, nn.Linear)] + [self.head]
        return [self.sigma] + [q for m in lin for q in (m.weight, m.bias)]

    def turn_on_body_grads(self):
        self.features_no_grad = False

    def turn_off_body_grads(self):
        self.features_no_grad = True
