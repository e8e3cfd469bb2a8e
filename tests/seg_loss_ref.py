"""Reference for the fused segmentation tail with a recipe (mv_seg_loss_*; contract in include/myrtle_vision_hip.h), composed from
torch ops in a chosen dtype: ``F.interpolate`` (bilinear, align_corners=False) plus the formulas

    CE   = [(1-eps) sum_valid w_y (lse - z_y) + (eps/C) sum_valid sum_c w_c (lse - z_c)] / W,   W = sum_valid w_y
    Dice = 1 - (1/C) sum_c (2 I_c + s) / (P_c + N_c + s)
    loss = CE + lam Dice

and the areas of ``utils.miou.intersect_and_union`` by ``bincount``.  Shared by tests/test_seg_loss_cpu.py (the formulas against
``F.cross_entropy`` and autograd, fp64) and tests/test_seg_loss_gpu.py (the kernels against this in fp64, under a bar measured on this
in fp32).  Inputs come from seeds; nothing here touches a GPU."""
import math

import torch
import torch.nn.functional as F

IGNORE = -100

# B, C, h, w, H, W, seed: the smallest shapes at which the kernels can go wrong
SHAPES = [
    (3, 17, 3, 4, 33, 35, 5),          # two forward blocks per image, the second ragged (1155 pixels); non-square, fractional scale
    (1, 32, 2, 2, 5, 257, 1000),       # the class limit; W > 256: the backward's column loop runs twice
    (2, 2, 6, 6, 6, 6, 2000),          # identity scale; smallest C
    (2, 5, 2, 2, 4, 4, 3000),          # integer scale; fewer pixels than one wave
]
SHAPE_IDS = [f"B{s[0]}-C{s[1]}-{s[2]}x{s[3]}-to-{s[4]}x{s[5]}" for s in SHAPES]
WORKLOAD_SHAPE = (2, 17, 14, 14, 224, 224, 7)

# name -> (class weights?, eps, lam, s)
OPTIONS = {
    "none": (False, 0.0, 0.0, 1.0),
    "weights": (True, 0.0, 0.0, 1.0),
    "smoothing": (False, 0.1, 0.0, 1.0),
    "dice": (False, 0.0, 0.5, 1.0),
    "all": (True, 0.1, 0.5, 1.0),
}
LABELINGS = ["valid", "ignored", "absent_class", "zero_weight_class", "all_zero_weight", "all_ignored", "out_of_range"]


def f32(v):
    """The fp32 value the kernels receive for a Python float."""
    return float(torch.tensor(v, dtype=torch.float32))


def make_small(B, C, h, w, seed):
    """fp32 [B, h*w, C]: 3 * randn from the seed (drawn in fp64, rounded once: with this draw every pixel of every shape of SHAPES
    keeps an fp64 arg-max margin above 1e-3, which tests/test_seg_loss_cpu.py asserts)."""
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(B, h * w, C, generator=g, dtype=torch.float64)).float()


def make_labels(B, C, H, W, seed, labeling):
    """int64 [B, H, W] and fp32 class weights [C] (for the runs that use weights) for one of LABELINGS."""
    g = torch.Generator().manual_seed(seed + 17)
    y = torch.randint(0, C, (B, H, W), generator=g)
    wts = 0.25 + 1.5 * torch.rand(C, generator=g)
    if labeling == "ignored":                               # a scatter of -100, and one whole image (where there is more than one)
        y[torch.rand(B, H, W, generator=g) < 0.2] = IGNORE
        y[B - 1] = IGNORE if B > 1 else y[B - 1]
        y[0, 0, 0] = IGNORE
    elif labeling == "absent_class":
        y[y == C - 1] = 0
    elif labeling == "zero_weight_class":
        wts[min(1, C - 1)] = 0.0
        y[0, 0, 0] = min(1, C - 1)                         # ... and present
    elif labeling == "all_zero_weight":                     # every PRESENT label's weight is 0: only class 0 is present
        y[:] = 0
        wts[0] = 0.0
    elif labeling == "all_ignored":
        y[:] = IGNORE
    elif labeling == "out_of_range":
        y[0, H - 1, W // 2] = C
    return y, wts


def upsample(small, B, C, h, w, H, W, dtype):
    """small [B, h*w, C] -> z [B, C, H, W] in ``dtype``."""
    return F.interpolate(small.to(dtype).view(B, h, w, C).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)


def masks(y, C):
    valid = (y >= 0) & (y < C)
    return valid, (~valid) & (y != IGNORE)


def terms(z, y, wts, eps, lam, s):
    """-> dict of tensors in z's dtype: ce, dice, loss (finite wherever the denominators are; the NaN rules are applied by
    ``reference``), W, P, I, N, a, b.  Differentiable in z.  Labels outside [0, C) take no part."""
    B, C, H, W_ = z.shape
    valid, _ = masks(y, C)
    zf = z.permute(0, 2, 3, 1).reshape(-1, C)[valid.reshape(-1)]                    # [n, C]
    yv = y.reshape(-1)[valid.reshape(-1)]
    wts = torch.ones(C, dtype=z.dtype) if wts is None else wts.to(z.dtype)
    lse = torch.logsumexp(zf, dim=1, keepdim=True)
    nlp = lse - zf                                                                   # -log p
    onehot = F.one_hot(yv, C).to(z.dtype) if yv.numel() else zf.new_zeros(0, C)
    wy = wts[yv]
    Wsum = wy.sum()
    num = (1.0 - eps) * (wy * (nlp * onehot).sum(1)).sum() + (eps / C) * (nlp * wts).sum()
    ce = num / Wsum
    p = torch.exp(-nlp)
    I, P, N = (p * onehot).sum(0), p.sum(0), onehot.sum(0)
    U = P + N + s
    dice = 1.0 - ((2.0 * I + s) / U).sum() / C if lam > 0 else zf.new_zeros(())
    return dict(ce=ce, dice=dice, loss=ce + lam * dice if lam > 0 else ce, W=Wsum, P=P, I=I, N=N,
                a=-(2.0 / C) / U, b=(2.0 * I + s) / (U * U) / C)


def analytic_dz(z, y, wts, eps, lam, s):
    """The per-pixel gradient of the specification -> [B, C, H, W], zero at pixels that are not valid."""
    B, C, H, W_ = z.shape
    valid, _ = masks(y, C)
    t = terms(z, y, wts, eps, lam, s)
    wts = torch.ones(C, dtype=z.dtype) if wts is None else wts.to(z.dtype)
    zl = z.permute(0, 2, 3, 1)                                                       # [B, H, W, C]
    p = torch.softmax(zl, dim=-1)
    yc = y.clamp(0, C - 1)
    onehot = F.one_hot(yc, C).to(z.dtype)
    wy = wts[yc].unsqueeze(-1)
    dz = (p * ((1.0 - eps) * wy + (eps / C) * wts.sum()) - (1.0 - eps) * wy * onehot - (eps / C) * wts) / t["W"]
    if lam > 0:
        g = t["a"] * onehot + t["b"]
        dz = dz + lam * p * (g - (p * g).sum(-1, keepdim=True))
    return (dz * valid.unsqueeze(-1).to(z.dtype)).permute(0, 3, 1, 2)


def areas(pred, y, C):
    """int64 [3, C] = (intersect | pred | label), utils.miou.intersect_and_union's semantics: pred over all pixels, labels outside
    [0, C) dropped."""
    pred, y = pred.reshape(-1).long(), y.reshape(-1).long()
    valid = (y >= 0) & (y < C)
    return torch.stack([torch.bincount(pred[pred == y], minlength=C), torch.bincount(pred, minlength=C),
                        torch.bincount(y[valid], minlength=C)])


def reference(small, y, dims, wts, eps, lam, s, dtype):
    """Everything the kernels return, from the torch composition in ``dtype`` -> dict: stats (8 Python floats, the NaN rules of the
    header applied), coef [2, C], dsmall [B*h*w, C] (autograd through the interpolation; the gradient of the loss with labels outside
    [0, C) left out, zero when W == 0), lse / pred [B, H, W], margin (smallest gap between the two largest logits of a pixel),
    areas int64 [3, C]."""
    B, C, h, w, H, W_ = dims
    eps, lam, s = f32(eps), f32(lam), f32(s)
    sm = small.to(dtype).clone().requires_grad_()
    z = upsample(sm, B, C, h, w, H, W_, dtype)
    valid, bad = masks(y, C)
    t = terms(z, y, wts, eps, lam, s)
    live = float(t["W"].detach()) > 0.0
    if live:
        t["loss"].backward()
        dsmall = sm.grad.reshape(B * h * w, C)
    else:
        dsmall = torch.zeros(B * h * w, C, dtype=dtype)
    t = {k: v.detach() for k, v in t.items()}
    zd = z.detach()
    top2 = zd.topk(2, dim=1).values
    pred = zd.argmax(dim=1)
    nan = float("nan")
    ce = nan if (not live or bool(bad.any())) else float(t["ce"])
    dice = float(t["dice"].detach()) if lam > 0 else 0.0
    stats = [ce + lam * dice if lam > 0 else ce, float((pred == y).double().mean()), float(valid.sum()), float(bad.sum()), ce, dice,
             float(t["W"]), 0.0]
    coef = torch.stack([t["a"], t["b"]]).detach() if lam > 0 else torch.zeros(2, C, dtype=dtype)
    return dict(stats=stats, coef=coef, dsmall=dsmall.detach(), lse=torch.logsumexp(zd, dim=1), pred=pred,
                margin=float((top2[:, 0] - top2[:, 1]).min()), areas=areas(pred, y, C))


# ---- the bar: 8 x the error of this composition in fp32 against fp64, never below 4 fp32 ulps of the value's magnitude --------------
def ulp32(x):
    """One fp32 unit in the last place at magnitude |x| (that of the smallest normal number below it)."""
    x = abs(float(x))
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23) if x > 0.0 and math.isfinite(x) else 2.0 ** -149


def scalar_bar(ref32, ref64):
    return max(8.0 * abs(ref32 - ref64), 4.0 * ulp32(ref64))


def tensor_bar(ref32, ref64):
    """For a tensor: the largest elementwise error against 8 x torch's largest elementwise error, floor 4 ulps of the largest
    magnitude."""
    return max(8.0 * float((ref32.double() - ref64).abs().max()), 4.0 * ulp32(float(ref64.abs().max())))
