"""What tests/test_mixup_cpu.py and tests/test_mixup_gpu.py share: seeded inputs, the torch restatements of the soft target, of
Mixup and of CutMix, and the Mixup error bound.  Not a test module."""
import torch

MIX_SHAPES = [(2, 3, 16, 16), (3, 3, 30, 34), (5, 1, 7, 9), (4, 3, 224, 224)]
MIX_LAMS = [0.3, 0.73]


def mix_inputs(shape, dtype):
    """The batch of one mix_batch case (CPU): N(0, 1), rounded to ``dtype``.  The seed depends on the shape alone."""
    g = torch.Generator().manual_seed(1000 + shape[0] * 131 + shape[2] * 17 + shape[3])
    return torch.randn(shape, generator=g).to(dtype)


def lam_pair(lam):
    """(lam, 1 - lam) as the fp32 values the kernel uses, as Python floats."""
    l32 = torch.tensor(lam, dtype=torch.float32)
    return float(l32), float(torch.tensor(1.0, dtype=torch.float32) - l32)


def mixup_exact(x, lam):
    """-> (exact, scale): ``lam * x_i + (1 - lam) * x_j`` with j = B - 1 - i in fp64 from the stored inputs, and
    ``|lam * x_i| + |(1 - lam) * x_j|``.  For odd B the middle sample pairs with itself: exact == x there, up to fp64 rounding."""
    l, o = lam_pair(lam)
    a, b = x.double(), x.double().flip(0)
    return l * a + o * b, (l * a).abs() + (o * b).abs()


def mixup_bound(x, lam):
    """Two rounded fp32 products and one rounded fp32 sum are off by at most 2^-23 * (|lam*a| + |(1-lam)*b|) (each product by
    2^-24 of itself, the sum by 2^-24 of at most their magnitudes' sum); a factor 2 over that.  A bf16 batch adds 2^-8 * |exact|
    for the single rounding of the result to bf16: bf16 keeps 8 significant bits, so just above a power of two that rounding alone
    reaches 2^-8 of the value (2^-9 on average over a binade) -- this term has no slack of its own."""
    exact, scale = mixup_exact(x, lam)
    bound = 2.0 ** -22 * scale
    if x.dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * exact.abs()
    return exact, bound


def cutmix_ref(x, box):
    """The index composition: inside the box every sample takes its partner's pixels."""
    y0, y1, x0, x1 = box
    out = x.clone()
    out[:, :, y0:y1, x0:x1] = x.flip(0)[:, :, y0:y1, x0:x1]
    return out


def cutmix_boxes(H, W):
    return {"empty": (3, 3, 2, 5), "empty_cols": (1, 4, 2, 2), "whole": (0, H, 0, W), "pixel": (1, 2, 1, 2), "top": (0, 2, 1, 3),
            "bottom": (H - 2, H, 1, 3), "left": (1, 3, 0, 2), "right": (1, 3, W - 2, W), "odd": (1, H - 1, 1, 4)}


def soft_target(labels, C, lam, eps):
    """t_i = lam * s(y_i) + (1 - lam) * s(y_j), j = B - 1 - i, s(y) = eps / C everywhere plus (1 - eps) at y; fp64 [B, C]."""
    s = torch.full((labels.numel(), C), eps / C, dtype=torch.float64)
    s[torch.arange(labels.numel()), labels] += 1.0 - eps
    return lam * s + (1.0 - lam) * s.flip(0)


def ce_inputs(B, C, scale=3.0):
    g = torch.Generator().manual_seed(7 * B + C)
    return torch.randn(B, C, generator=g) * scale, torch.randint(0, C, (B,), generator=g)
