"""Per-parameter inner-loop step sizes for ``MAML``: one step per model (``per='scalar'``), per parameter tensor (``'tensor'``) or
per entry (``'parameter'``), optionally one set per inner step, optionally learnable (learn2learn's ``MetaSGD`` beside ``MAML``),
with tensors frozen by name prefix (the MAML-against-ANIL question: which layers have to adapt).

``MAML(model, lr=InnerLR(model, 0.5, per='tensor', learnable=True))``: the fused call (``fast_adapt`` / ``meta_batch_adapt``) takes the
step sizes as one vector per inner step (``MetaEngine.meta_batch_lr``) and ``.backward()`` fills their ``.grad`` next to the
model's; the step-wise learner (``learner.adapt``) applies ``theta - lr_flat * g``, which autograd differentiates.
"""
import torch


class InnerLR(torch.nn.Module):
    def __init__(self, model, init, per='tensor', steps=1, learnable=False, frozen=()):
        """model: the module whose ``named_parameters()`` the step sizes follow.  init: the initial step size (a number, or a tensor
        broadcastable to the stored shape: [steps, 1] / [steps, tensors] / [steps, P]).  steps: 1 = the same step sizes for every
        inner step, K = one set per inner step of a K-step adaptation.  frozen: parameter-name prefixes (``'base.0.'``, ``'linear.'``)
        whose step size is pinned to 0: not adapted, and no gradient reaches the stored value."""
        super().__init__()
        if per not in ('scalar', 'tensor', 'parameter'):
            raise ValueError(f"per must be 'scalar', 'tensor' or 'parameter', got {per!r}")
        if int(steps) < 1:
            raise ValueError(f'steps must be >= 1, got {steps}')
        named = list(model.named_parameters())
        if not named:
            raise ValueError('the model has no parameters')
        self.per, self.steps, self.learnable = per, int(steps), bool(learnable)
        self.frozen = tuple(frozen)
        self.names = [n for n, _ in named]
        self.sizes = [p.numel() for _, p in named]
        for pre in self.frozen:
            if not any(n.startswith(pre) for n in self.names):
                raise ValueError(f'frozen prefix {pre!r} matches no parameter of the model ({self.names[0]} ... {self.names[-1]})')
        width = {'scalar': 1, 'tensor': len(named), 'parameter': sum(self.sizes)}[per]
        dev = named[0][1].device
        values = torch.empty(self.steps, width, dtype=torch.float32, device=dev)
        values.copy_(torch.as_tensor(init, dtype=torch.float32, device=dev).expand(self.steps, width) if torch.is_tensor(init)
                     else torch.full((self.steps, width), float(init), dtype=torch.float32, device=dev))
        if self.learnable:
            self.values = torch.nn.Parameter(values)
        else:
            self.register_buffer('values', values)

    def is_frozen(self, name):
        return any(name.startswith(pre) for pre in self.frozen)

    def flat(self, also_frozen=()):
        """[steps, P] step sizes in ``model.parameters()`` order, connected to ``values`` by expand / cat (a per-tensor step receives
        the sum of its entries' gradients).  Frozen tensors, and those named in ``also_frozen``, are zeros."""
        v, pieces, off = self.values, [], 0
        also = set(also_frozen)
        for i, (name, n) in enumerate(zip(self.names, self.sizes)):
            if self.is_frozen(name) or name in also:
                pieces.append(v.new_zeros(self.steps, n))
            elif self.per == 'scalar':
                pieces.append(v.expand(self.steps, n))
            elif self.per == 'tensor':
                pieces.append(v[:, i:i + 1].expand(self.steps, n))
            else:
                pieces.append(v[:, off:off + n])
            off += n
        return torch.cat(pieces, dim=1)

    def extra_repr(self):
        return f"per={self.per!r}, steps={self.steps}, learnable={self.learnable}, frozen={self.frozen}"
