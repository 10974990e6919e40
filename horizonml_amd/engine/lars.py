"""LARS in plain torch: the segmented fused step's contract, per parameter.

This is the eager / CPU-gloo engine's optimizer for ``--lars`` and, run on
float64 parameters, the reference the GPU tests hold ``k_sgd_step_seg``
against — one definition, the way the augment hash has a Python mirror.

Per step, over every parameter ``s`` of every group (docs/KERNELS.md,
"Segmented step"):

1. ``G_s = sum(g*g)``, ``W_s = sum(w*w)``; ``N = sqrt(sum_s G_s)``, summed in
   parameter order.
2. ``c = 1`` when ``max_norm <= 0``, else ``min(1, max_norm / (N + 1e-6))``.
3. ``wd_s`` is the group's ``weight_decay`` (a no-decay group carries 0).
4. For ``ndim > 1`` (``adapt_s = 1``), with ``|g| = c*sqrt(G_s)`` and
   ``|w| = sqrt(W_s)``: ``q_s = eta*|w| / (|g| + wd_s*|w| + 1e-8)`` when both
   norms are positive, else 1.  ``ndim <= 1``: ``q_s = 1``.
5. ``g' = (q_s*c)*g + (q_s*wd_s)*w``; then SGD momentum as ``torch.optim.SGD``
   defines it: ``u = mu*buf + g'``, ``w -= lr*(g' + mu*u)`` with Nesterov,
   ``w -= lr*u`` without.

All arithmetic runs in the parameters' dtype.
"""
from __future__ import annotations

import torch


class LARS(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 0.1, momentum: float = 0.9,
                 weight_decay: float = 0.0, nesterov: bool = False,
                 eta: float = 1e-3, max_norm: float = 0.0):
        if nesterov and not momentum > 0:
            raise ValueError("nesterov needs momentum > 0")
        if eta <= 0 or max_norm < 0:
            raise ValueError("eta must be > 0 and max_norm >= 0")
        super().__init__(params, dict(lr=lr, momentum=momentum,
                                      weight_decay=weight_decay,
                                      nesterov=nesterov, eta=eta))
        self.max_norm = float(max_norm)
        self.grad_norm = None  # N of the last step (a 0-d tensor)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        todo = [(group, p) for group in self.param_groups
                for p in group["params"] if p.grad is not None]
        if not todo:
            return loss
        G = [(p.grad * p.grad).sum() for _, p in todo]
        total = G[0].clone()
        for g_s in G[1:]:
            total = total + g_s.to(total)
        N = total.sqrt()
        self.grad_norm = N
        c = torch.ones_like(N)
        if self.max_norm > 0:
            c = torch.clamp(self.max_norm / (N + 1e-6), max=1.0)
        for (group, p), G_s in zip(todo, G):
            c_p = c.to(p)
            wd, mu = group["weight_decay"], group["momentum"]
            q = torch.ones_like(c_p)
            if p.ndim > 1:
                gn = c_p * G_s.sqrt()
                wn = (p * p).sum().sqrt()
                if float(wn) > 0 and float(gn) > 0:
                    q = group["eta"] * wn / (gn + wd * wn + 1e-8)
            g = (q * c_p) * p.grad
            if wd != 0:
                g = g + (q * wd) * p
            if mu > 0:
                state = self.state[p]
                if "momentum_buffer" not in state:
                    state["momentum_buffer"] = torch.zeros_like(p)
                u = state["momentum_buffer"].mul_(mu).add_(g)
                g = g + mu * u if group["nesterov"] else u
            p.add_(g, alpha=-group["lr"])
        return loss
