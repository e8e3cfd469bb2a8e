"""Shared reference of the ``mv_adamw_table`` tests: ``torch.optim.AdamW`` on the CPU with ONE param group per tensor
(``lr = scheduled lr x that tensor's scale``, that tensor's weight decay) and the EMA recurrence evaluated in fp64; plus the edge
arena both test files cut into items."""
import torch

# the project's AdamW bar (tests/test_hip_ops.py::test_adamw_matches_torch): max |got - want| / max |want| over an array
BAR = 2e-6
ITEM_MAX = 4096
EDGE_SIZES = [1, 3, 5, 7, 8, 9, 4095, 4096, 4097, 8197, 70001]


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def arena_offsets(sizes):
    """``ParamArena``'s layout rule: every tensor starts on a multiple of 8 elements -> (offsets, total)."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 7) & ~7
    return offs, total


def gap_mask(offsets, sizes, total):
    """bool [total]: True on the alignment-gap elements that belong to no tensor."""
    mask = torch.ones(total, dtype=torch.bool)
    for o, n in zip(offsets, sizes):
        mask[o:o + n] = False
    return mask


def edge_arena(count=40):
    """About 40 tensors cycling through EDGE_SIZES -> (sizes, offsets, total)."""
    sizes = [EDGE_SIZES[i % len(EDGE_SIZES)] for i in range(count)]
    offs, total = arena_offsets(sizes)
    return sizes, offs, total


def flat(tensors, offsets, total, dtype=torch.float32):
    out = torch.zeros(total, dtype=dtype)
    for t, o in zip(tensors, offsets):
        out[o:o + t.numel()] = t.reshape(-1).to(dtype)
    return out


class Reference:
    """``torch.optim.AdamW`` over CPU copies of the tensors, one group per tensor, and the fp64 EMA of its weights."""

    def __init__(self, tensors, scales, wds, betas=(0.9, 0.999), eps=1e-8, ema_decay=None):
        self.params = [torch.nn.Parameter(t.detach().float().cpu().clone()) for t in tensors]
        self.scales = [float(s) for s in scales]
        self.opt = torch.optim.AdamW([{"params": [p], "lr": 1.0, "weight_decay": float(w)} for p, w in zip(self.params, wds)],
                                     lr=1.0, betas=betas, eps=eps)
        self.ema_decay = ema_decay
        self.ema = [p.detach().double().clone() for p in self.params] if ema_decay is not None else None

    def step(self, lr, grads):
        """One step at the scheduled rate ``lr`` with the gradients ``grads`` (what the kernel multiplies in -- grad_scale, the clip
        coefficient -- already applied by the caller, in fp32 as the kernel does)."""
        for group, s in zip(self.opt.param_groups, self.scales):
            group["lr"] = lr * s
        for p, g in zip(self.params, grads):
            p.grad = g.detach().float().cpu().reshape(p.shape).clone()
        self.opt.step()
        if self.ema is not None:
            d = float(torch.tensor(self.ema_decay, dtype=torch.float32))     # the decay the kernel is handed: an fp32 argument
            self.ema = [d * e + (1.0 - d) * p.detach().double() for e, p in zip(self.ema, self.params)]
