"""Shared references of the ``mv_sgd_table`` / ``mv_lamb_table`` tests, on the CPU.  SGD: ``torch.optim.SGD`` with ONE param group per
tensor (``lr = scheduled lr x that tensor's scale``, that tensor's weight decay), as ``optim_table_ref.Reference`` does for AdamW.
LAMB: the formulas of ``utils.optim.TableLamb``'s docstring in plain torch, dtype-generic -- fp64 is the checker, fp32 the baseline
whose own error against fp64 sets the bar for the kernel (8 x, the project's rule for a kernel against a torch composition, never
below ``BAR``).  Not a test module (no test_ prefix): imported by them."""
import torch

from optim_table_ref import BAR, EDGE_SIZES, ITEM_MAX, arena_offsets, edge_arena, flat, gap_mask, relerr  # noqa: F401

PARITY_FACTOR = 8
BIG = 256 * ITEM_MAX + 1                                      # more items than a workgroup has threads


def f32(x):
    """The value an fp32 argument or table entry of the C ABI holds."""
    return float(torch.tensor(x, dtype=torch.float32))


class SGDReference:
    """``torch.optim.SGD`` (dampening 0) over CPU copies of the tensors, one group per tensor."""

    def __init__(self, tensors, scales, wds, momentum, nesterov):
        self.params = [torch.nn.Parameter(t.detach().float().cpu().clone()) for t in tensors]
        self.scales = [float(s) for s in scales]
        self.opt = torch.optim.SGD([{"params": [p], "lr": 1.0, "weight_decay": float(w)} for p, w in zip(self.params, wds)],
                                   lr=1.0, momentum=momentum, dampening=0, nesterov=nesterov)

    def step(self, lr, grads):
        """One step at the scheduled rate ``lr``; ``grads`` already carry what the kernel multiplies in (fp32, as the kernel does)."""
        for group, s in zip(self.opt.param_groups, self.scales):
            group["lr"] = lr * s
        for p, g in zip(self.params, grads):
            p.grad = g.detach().float().cpu().reshape(p.shape).clone()
        self.opt.step()

    def buffers(self):
        return [self.opt.state[p].get("momentum_buffer") for p in self.params]


class LambReference:
    """``TableLamb``'s formulas in ``dtype`` (torch.float64: the checker; torch.float32: the baseline).  Every scalar is first rounded
    to the fp32 the kernel is handed (rates, scales, decays, betas, eps, the bias corrections formed on the host in double as
    ``ops.lamb_table_step`` forms them), so both evaluations and the kernel start from the same numbers."""

    def __init__(self, tensors, scales, wds, betas=(0.9, 0.999), eps=1e-6, dtype=torch.float64):
        self.dtype = dtype
        self.p = [t.detach().cpu().to(dtype).clone() for t in tensors]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.scales, self.wds = [f32(s) for s in scales], [f32(w) for w in wds]
        self.betas, self.b1, self.b2, self.eps = betas, f32(betas[0]), f32(betas[1]), f32(eps)
        self.t = 0
        self.trust = []

    def step(self, lr, grads):
        self.t += 1
        lr = f32(lr)
        bc1, bc2 = f32(1.0 - self.betas[0] ** self.t), f32(1.0 - self.betas[1] ** self.t)
        b1, b2, eps = self.b1, self.b2, self.eps
        self.trust = []
        for j, g in enumerate(grads):
            g = g.detach().cpu().to(self.dtype).reshape(self.p[j].shape)
            p, wd = self.p[j], self.wds[j]
            self.m[j] = b1 * self.m[j] + (1.0 - b1) * g
            self.v[j] = b2 * self.v[j] + (1.0 - b2) * g * g
            u = (self.m[j] / bc1) / (self.v[j].sqrt() / bc2 ** 0.5 + eps) + wd * p
            wn, un = float(p.norm()), float(u.norm())
            trust = wn / un if (wd != 0 and wn > 0 and un > 0) else 1.0
            self.trust.append(trust)
            self.p[j] = p - (lr * self.scales[j] * trust) * u


def lamb_bars(ref64, ref32):
    """Per tensor: (the fp32 evaluation's error against fp64, the bar for the kernel's p = max(BAR, 8 x that))."""
    out = []
    for a, b in zip(ref32.p, ref64.p):
        base = relerr(a, b)
        out.append((base, max(BAR, PARITY_FACTOR * base)))
    return out
