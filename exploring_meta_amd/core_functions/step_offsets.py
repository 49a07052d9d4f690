"""Per-step parameter offsets for ``MAML``: inner step ``j`` ends in ``theta - lr * g + s_j``, with the rows ``s_1 .. s_K`` shared by
all tasks and, when learnable, meta-learned with the model.  On the BatchNorm tensors (``tensors='bn'``) this is MAML++'s per-step
BatchNorm weights and biases (Antoniou et al., 2019) in cumulative parametrisation: with the BatchNorm tensors out of the inner loop
(``InnerLR(frozen=offsets.bn_prefixes())``) step ``j`` sees ``gamma + s_1 + .. + s_j``, the model's own gamma / beta serve step 0, and a
zero-initialised run starts as plain MAML.

``MAML(model, lr, offsets=StepOffsets(model, K))``: the fused call (``fast_adapt`` / ``meta_batch_adapt`` / ``meta_batch_adapt_steps``)
takes the rows as one ``[K, P]`` tensor (``MetaEngine.meta_batch_offsets``) and ``.backward()`` fills their ``.grad`` next to the model's;
the step-wise learner (``learner.adapt``) adds the row of the step it is at, which autograd differentiates.
"""
import torch


class StepOffsets(torch.nn.Module):
    def __init__(self, model, steps, tensors='bn', learnable=True, init=0.0):
        """model: the module whose ``named_parameters()`` the offsets follow.  steps: the number of inner steps K (one row each).
        tensors: ``'bn'`` = the tensors whose name contains ``.normalize.``; ``'all'``; or an iterable of parameter-name prefixes
        (``'base.0.'``, ``'linear.bias'``), as ``InnerLR.frozen`` takes.  init: the initial value (a number, or a tensor broadcastable
        to ``[steps, width]``, width = the selected tensors' entries)."""
        super().__init__()
        if isinstance(steps, bool) or int(steps) != steps or int(steps) < 1:
            raise ValueError(f'steps must be an integer >= 1, got {steps!r}')
        named = list(model.named_parameters())
        if not named:
            raise ValueError('the model has no parameters')
        self.steps, self.learnable = int(steps), bool(learnable)
        self.names = [n for n, _ in named]
        self.sizes = [p.numel() for _, p in named]
        if isinstance(tensors, str):
            if tensors not in ('bn', 'all'):
                raise ValueError(f"tensors must be 'bn', 'all' or an iterable of parameter-name prefixes, got {tensors!r}")
            self.selected = [tensors == 'all' or '.normalize.' in n for n in self.names]
            if not any(self.selected):
                raise ValueError("tensors='bn' matches no parameter of the model: none is named '.normalize.'")
        else:
            prefixes = tuple(tensors)
            for pre in prefixes:
                if not isinstance(pre, str) or not any(n.startswith(pre) for n in self.names):
                    raise ValueError(f'prefix {pre!r} matches no parameter of the model ({self.names[0]} ... {self.names[-1]})')
            if not prefixes:
                raise ValueError('no tensor selected')
            self.selected = [any(n.startswith(pre) for pre in prefixes) for n in self.names]
        self.tensors = tensors if isinstance(tensors, str) else prefixes
        width = sum(n for n, sel in zip(self.sizes, self.selected) if sel)
        dev = named[0][1].device
        values = torch.empty(self.steps, width, dtype=torch.float32, device=dev)
        values.copy_(torch.as_tensor(init, dtype=torch.float32, device=dev).expand(self.steps, width) if torch.is_tensor(init)
                     else torch.full((self.steps, width), float(init), dtype=torch.float32, device=dev))
        if self.learnable:
            self.values = torch.nn.Parameter(values)
        else:
            self.register_buffer('values', values)

    def flat(self):
        """[steps, P] offsets in ``model.parameters()`` order: zeros on the tensors that are not selected, connected to ``values`` by
        cat, so autograd routes the gradient of the selected columns to ``values``."""
        v, pieces, off = self.values, [], 0
        for n, sel in zip(self.sizes, self.selected):
            if sel:
                pieces.append(v[:, off:off + n])
                off += n
            else:
                pieces.append(v.new_zeros(self.steps, n))
        return torch.cat(pieces, dim=1)

    def rows(self):
        """The cumulative sums s_1 + .. + s_j, [steps, P]: what step j has added to a tensor that the inner loop leaves alone."""
        return torch.cumsum(self.flat().detach(), dim=0)

    def bn_prefixes(self):
        """The selected tensors' names as prefixes, for freezing them in an ``InnerLR`` (``frozen=offsets.bn_prefixes()``)."""
        return tuple(n for n, sel in zip(self.names, self.selected) if sel)

    def extra_repr(self):
        return f"steps={self.steps}, tensors={self.tensors!r}, learnable={self.learnable}"
