"""``MAML`` wrapper with the call surface of the reference's ``core_functions/maml.py`` (a learn2learn ``MAML`` subclass),
without the learn2learn dependency.

``maml = MAML(model, lr, first_order=False)``; ``learner = maml.clone()``; ``fast_adapt(batch, learner, ...)``;
``eval_loss.backward()`` accumulates into ``maml.parameters()``'s ``.grad`` exactly like the reference loop
(vision/maml_vision.py:84,104-112).  A clone does not copy tensors: it records the base module, and the fused HIP engine
starts every task from the base parameters (the semantics of learn2learn's ``clone_module``).

The step-wise surface (``learner(x)``, ``learner.adapt(loss)``, ``get_rep``, ``get_rep_i`` -- what the reference's
misc_scripts/cl_vision.py and rc_vision.py drive) holds the fast weights as one flat tensor and runs every forward /
gradient through ``mi_learner_forward`` / ``mi_learner_backward``.

Around a policy (``DiagNormalPolicy`` / ``DiagNormalPolicyANIL``) the wrapper is a step-wise learner too (the reference's
misc_scripts/cl_rl.py:71-75: ``learner.adapt(vpg_a2c_loss(episodes, learner, ...))``): ``learner.log_prob`` / ``learner.density``
run on the fast weights through ``mi_policy_forward`` / ``mi_policy_vjp`` / ``mi_policy_hvp`` whenever a graph is wanted (grad mode
on and parameters that require grad) or the learner has been adapted.  ``learner(state)`` samples and never builds a graph; a
learner that was never adapted acts through the bare policy exactly as before.

``lr`` is a number (the reference's scalar step, today's scalar fused call) or an ``InnerLR`` (inner_lr.py): step sizes per tensor /
per entry / per inner step, learnable or not.  A learnable ``InnerLR`` is a submodule, so its values are among ``maml.parameters()``
(learn2learn ``MetaSGD``).  ``allow_nograd=True`` gives parameters with ``requires_grad=False`` the step 0, in the fused call and in
``adapt`` (learn2learn's ``adapt`` skips them).

``offsets`` is ``None`` or a ``StepOffsets`` (step_offsets.py): per-step parameter offsets, ``theta - lr * g + s_j`` after inner step j --
MAML++'s per-step BatchNorm weights and biases.  It is a submodule too: a learnable one is among ``maml.parameters()``.
"""
import copy


import torch

from .inner_lr import InnerLR
from .step_offsets import StepOffsets


class MAML(torch.nn.Module):
    def __init__(self, model, lr, first_order=False, allow_unused=None, allow_nograd=False, offsets=None):
        super().__init__()
        if offsets is not None and not isinstance(offsets, StepOffsets):
            raise TypeError(f'offsets must be a StepOffsets or None, got {type(offsets).__name__}')
        self.module = model
        self.lr = lr                       # a number, or an InnerLR (a submodule: parameters when learnable, a buffer otherwise)
        self.offsets = offsets             # None, or a StepOffsets (a submodule likewise)
        self.first_order = first_order
        self.allow_nograd = allow_nograd
        self.allow_unused = allow_nograd if allow_unused is None else allow_unused
        self.__dict__['_fast'] = None      # flat fast weights of a step-wise learner (plain tensor, not a Parameter)
        self.__dict__['_steps_done'] = 0   # inner steps this learner has taken (selects the row of per-step sizes)

    def __getattr__(self, attr):
        try:
            return super().__getattr__(attr)
        except AttributeError:
            return getattr(self.__dict__['_modules']['module'], attr)

    def fast_weights(self):
        """Flat fast weights (parameters() order), connected to the base parameters in the autograd graph."""
        if self.__dict__['_fast'] is None:
            self.__dict__['_fast'] = self.module.flat_parameters()
        return self.__dict__['_fast']

    def lr_flat(self):
        """None while the step size is one number for every parameter (the scalar fused call); else the step sizes [steps, P] in
        ``parameters()`` order (around a policy: the engine's order, ``_engine_order``): an ``InnerLR``'s, with zeros for parameters
        that do not require grad under ``allow_nograd``."""
        lr = self.lr
        nograd = [n for n, p in self.module.named_parameters() if not p.requires_grad] if self.allow_nograd else []
        if isinstance(lr, InnerLR):
            return self._engine_order(lr.flat(also_frozen=nograd))
        if not nograd:
            return None
        return self._engine_order(torch.cat([torch.full((p.numel(),), 0.0 if not p.requires_grad else float(lr), dtype=torch.float32,
                                                        device=p.device) for p in self.module.parameters()]).unsqueeze(0))

    def offsets_flat(self):
        """None without per-step offsets; else the offsets [steps, P] in ``parameters()`` order (``StepOffsets.flat``)."""
        return None if self.offsets is None else self.offsets.flat()

    def _step_offset(self):
        """The row of offsets this learner's next ``adapt`` adds after its update, or None."""
        flat = self.offsets_flat()
        if flat is None:
            return None
        k = self.__dict__['_steps_done']
        if k >= flat.shape[0]:
            raise RuntimeError(f'this learner holds offsets for {flat.shape[0]} inner steps and has taken {k}')
        return flat[k]

    def _engine_order(self, flat):
        """Around a policy the step sizes leave in the ENGINE's parameter order (``_engine_params()``: sigma first), which is the order
        of the fast weights and of the fused policy calls.  ``InnerLR.flat()`` follows ``named_parameters()``; for ``DiagNormalPolicy`` and
        ``DiagNormalPolicyANIL`` that is the same order (a module's own parameters, ``sigma``, come before its children's), and nothing is
        moved.  A policy that registers its parameters in another order (``sigma`` held by a child module, say) gets one differentiable
        gather with an index built once from ``_engine_params()``, so gradients still reach ``InnerLR.values``.  Other modules: unchanged."""
        if not self._is_policy():
            return flat
        perm = self.__dict__.get('_lr_perm')
        if perm is None:
            start, off = {}, 0
            for p in self.module.parameters():
                start[id(p)] = off
                off += p.numel()
            perm = torch.cat([torch.arange(start[id(q)], start[id(q)] + q.numel()) for q in self.module._engine_params()])
            if perm.numel() != off:
                raise RuntimeError(f'the policy has {off} parameters, its engine order names {perm.numel()}')
            if torch.equal(perm, torch.arange(off)):
                perm = False                              # DiagNormalPolicy(.ANIL): the two orders agree
            self.__dict__['_lr_perm'] = perm
        if perm is False:
            return flat
        if perm.device != flat.device:
            perm = self.__dict__['_lr_perm'] = perm.to(flat.device)
        return flat.index_select(1, perm)

    def _step_lr(self):
        """The step size(s) of this learner's next ``adapt``: the number, or the row of ``lr_flat`` for the step it is at."""
        flat = self.lr_flat()
        if flat is None:
            return self.lr
        k = self.__dict__['_steps_done']
        if flat.shape[0] > 1 and k >= flat.shape[0]:
            raise RuntimeError(f'this learner holds step sizes for {flat.shape[0]} inner steps and has taken {k}')
        return flat[k if flat.shape[0] > 1 else 0]

    def _is_policy(self):
        return hasattr(self.module, 'density') and hasattr(self.module, 'flat_parameters')

    def _policy_theta(self):
        """Fast weights for a policy call, or None for the bare (detached) policy: the fast weights once the learner has them (after
        ``adapt`` / ``fast_weights``), or the parameters themselves when the caller can differentiate the result."""
        fast = self.__dict__['_fast']
        if fast is not None:
            return fast
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.module.parameters()):
            return self.module.flat_parameters()          # not kept: a learner that was never adapted holds no state
        return None

    def forward(self, x):
        """`learner(x)`: the module evaluated with this learner's current fast weights (mi_learner_forward); for a policy, an action
        sampled from the density at the fast weights (no graph; the bare policy until the learner has fast weights)."""
        if self._is_policy():
            fast = self.__dict__['_fast']
            return self.module(x) if fast is None else self.module(x, theta=fast)
        if not hasattr(self.module, 'flat_parameters'):
            return self.module(x)
        return self.module(x, theta=self.fast_weights())

    def density(self, state):
        """policies.py:49-52 at this learner's fast weights (see ``_policy_theta``)."""
        theta = self._policy_theta()
        return self.module.density(state) if theta is None else self.module.density(state, theta=theta)

    def log_prob(self, state, action):
        """policies.py:54-56 at this learner's fast weights; differentiable to second order (mi_policy_vjp / mi_policy_hvp)."""
        theta = self._policy_theta()
        return self.module.log_prob(state, action) if theta is None else self.module.log_prob(state, action, theta=theta)

    def adapted_policy(self):
        """A detached copy of the policy holding this learner's current fast weights (for rollouts: runners act with a bare policy)."""
        pol = copy.deepcopy(self.module)
        fast = self.__dict__['_fast']
        if fast is not None:
            pol.load_flat(fast.detach().float().contiguous())
        return pol

    def __deepcopy__(self, memo):
        """nn.Module's default copy, with the fast weights (a graph node, which torch refuses to deep-copy) taken as detached values."""
        fast = self.__dict__['_fast']
        if fast is not None and not fast.is_leaf:
            memo[id(fast)] = fast.detach().clone()
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def clone(self, first_order=None, allow_unused=None, allow_nograd=None):
        """reference core_functions/maml.py:23-49 (learn2learn clone_module: the clone starts from the CURRENT weights of
        this learner and stays connected to them in the graph)."""
        if first_order is None:
            first_order = self.first_order
        if allow_unused is None:
            allow_unused = self.allow_unused
        if allow_nograd is None:
            allow_nograd = self.allow_nograd
        c = MAML(self.module, lr=self.lr, first_order=first_order, allow_unused=allow_unused, allow_nograd=allow_nograd, offsets=self.offsets)
        c.__dict__['_fast'] = self.__dict__['_fast']
        c.__dict__['_steps_done'] = self.__dict__['_steps_done']
        return c

    def adapt(self, loss, first_order=None, allow_unused=None, allow_nograd=None):
        """learn2learn `MAML.adapt` (call sites core_functions/vision.py:13, misc_scripts/cl_vision.py:59,
        rc_vision.py:70): g = grad(loss, fast weights); p <- p - lr * g, out of place.

        `loss` must come from `learner(x)` of this learner.  The gradient is one mi_learner_backward call.  The update keeps the
        identity path to the base parameters; a first-order learner detaches the gradient (first-order meta-gradient), a
        second-order one keeps it in the graph (create_graph) and a later `.backward()` differentiates through it with
        mi_learner_hvp -- the exact second-order meta-gradient, one Hessian-vector sweep per adapt step.  Training loops are
        faster through `fast_adapt` / `meta_batch_adapt` (one fused HIP call for the K steps, the query pass and the outer
        backward for a whole meta-batch)."""
        if first_order is None:
            first_order = self.first_order
        second_order = not first_order
        if allow_unused is None:
            allow_unused = self.allow_unused
        s = self._step_offset()            # theta - lr * g + s: the row of the step this learner is at (autograd differentiates it)
        if s is not None and self._is_policy():
            raise NotImplementedError('per-step offsets are implemented for the fused MAML vision call')
        if self.__dict__['_fast'] is None and self._is_policy():
            # first step of a policy learner: the loss came from the parameters themselves (``_policy_theta``)
            params = self.module._engine_params()
            gs = torch.autograd.grad(loss, params, retain_graph=second_order, create_graph=second_order, allow_unused=bool(allow_unused))
            g = torch.cat([(torch.zeros_like(p) if gi is None else gi).reshape(-1) for p, gi in zip(params, gs)])
            self.__dict__['_fast'] = self.module.flat_parameters() - self._step_lr() * g
            self.__dict__['_steps_done'] += 1
            return
        theta = self.fast_weights()
        if not theta.requires_grad:
            raise RuntimeError('learner.adapt needs parameters that require grad')
        (g,) = torch.autograd.grad(loss, theta, retain_graph=second_order, create_graph=second_order, allow_unused=bool(allow_unused))
        new = theta if g is None else theta - self._step_lr() * g
        self.__dict__['_fast'] = new if s is None else new + s
        self.__dict__['_steps_done'] += 1

    def get_rep(self, input_d):
        """reference core_functions/maml.py:15-16"""
        return self.module.get_base_representation(input_d, theta=self.fast_weights())

    def get_rep_i(self, input_d, layer_i):
        """reference core_functions/maml.py:18-19"""
        return self.module.get_rep_layer(input_d, layer_i, theta=self.fast_weights())
