"""Shared by tests/test_distill_cpu.py and tests/test_distill_gpu.py: the inputs of the distillation-loss cases, the fp64 oracle of
the formulas in include/myrtle_vision_hip.h (numpy, written from the formulas and from nothing else), torch's evaluation of the
reference expression (models/distill.py:142-151: ``F.cross_entropy`` + ``T^2 * F.kl_div(..., "batchmean")``) in a chosen precision,
and the tolerance rule.

The rule is the project's (profiles/detection_parity.txt): baseline = the largest error, over all cases, of torch's own fp32
evaluation of the same expression against fp64 on the same inputs, max|fp32 - fp64| / max|fp64| per quantity; bound = 8 x baseline
(the kernel sums in another order and is still fp32).  Nothing here is fixed in advance: ``baselines()`` computes the table when the
tests run.  ``python tests/distill_ref.py`` on a machine with the device prints the table with the kernel's measured errors beside
it (profiles/distill_parity.txt)."""
import functools
import itertools

import numpy as np
import torch
import torch.nn.functional as TF

BATCHES = (1, 2, 7, 64)
CLASSES = (2, 45, 64, 65, 1000, 1001)      # one wave exactly, one past it, the reference's class count, ImageNet's (+1)
TEMPERATURES = (1.0, 3.0)
ALPHAS = (0.0, 0.5, 1.0)
MODES = ("soft", "hard")
LABELLINGS = ((1.0, 0.0, False), (0.3, 0.1, True))           # (lam, eps, pair_flip): plain labels, the Mixup recipe's
QUANTITIES = ("loss", "ce", "kd", "dstudent", "ddistill")
FACTOR = 8.0


def settings():
    return list(itertools.product(TEMPERATURES, ALPHAS, MODES, LABELLINGS))


@functools.lru_cache(maxsize=None)
def inputs(B, C):
    """-> (student, distill, teacher fp32 [B, C], labels int64 [B]) on the host.  The teacher's top-2 gap is positive in every row
    (fp32 and fp64 agree on its arg-max); from 45 classes on, one teacher logit of row 0 is so low that its softmax weight is
    exactly zero in fp32 and in fp64 (the p_c == 0 branch)."""
    g = torch.Generator().manual_seed(1000 * B + C)
    s, d, t = (2.0 * torch.randn(B, C, generator=g) for _ in range(3))
    if C >= 45:
        t[0, 5] = -1.0e4
    top = t.topk(2, dim=1).values
    t[torch.arange(B), t.argmax(1)] += (top[:, 0] - top[:, 1] < 1e-3).float()          # lift a near-tie clear of rounding
    y = torch.randint(0, C, (B,), generator=g)
    return s, d, t, y


def teacher_gap(t):
    top = t.topk(2, dim=1).values
    return float((top[:, 0] - top[:, 1]).min())


def _target(y, C, lam, eps, pair_flip, xp):
    """t_i = lam * s(y_i) + (1 - lam) * s(y_j), j = B - 1 - i, s(y) = eps / C everywhere plus (1 - eps) at y."""
    B = len(y)
    hot = xp.zeros((B, C))
    hot[xp.arange(B), y] = 1.0
    smooth = eps / C + (1.0 - eps) * hot
    return lam * smooth + (1.0 - lam) * smooth[::-1] if pair_flip else smooth


def _lse(z):
    m = z.max(axis=1, keepdims=True)
    return m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))


def oracle(s, d, t, y, T, alpha, mode, lam=1.0, eps=0.0, pair_flip=False, grad_scale=1.0):
    """fp64, from the formulas of the header -> dict of ``QUANTITIES`` (+ per-sample "ce_i", "kd_i")."""
    s, d, t = (np.asarray(v, dtype=np.float64) for v in (s, d, t))
    y = np.asarray(y)
    B, C = s.shape
    tgt = _target(y, C, lam, eps, pair_flip, np)
    logp_s = s - _lse(s)
    ce_i = -(tgt * logp_s).sum(axis=1)
    ds = alpha * (np.exp(logp_s) - tgt) * grad_scale / B
    if mode == "soft":
        logp, logq = t / T - _lse(t / T), d / T - _lse(d / T)
        p, q = np.exp(logp), np.exp(logq)
        kd_i = T * T * np.where(p > 0, p * (logp - logq), 0.0).sum(axis=1)
        dd = (1.0 - alpha) * T * (q - p) * grad_scale / B
    else:
        at = t.argmax(axis=1)                                   # first index wins
        kd_i = _lse(d)[:, 0] - d[np.arange(B), at]
        hot = np.zeros((B, C))
        hot[np.arange(B), at] = 1.0
        dd = (1.0 - alpha) * (np.exp(d - _lse(d)) - hot) * grad_scale / B
    ce, kd = ce_i.mean(), kd_i.mean()
    return dict(loss=alpha * ce + (1.0 - alpha) * kd, ce=ce, kd=kd, dstudent=ds, ddistill=dd, ce_i=ce_i, kd_i=kd_i)


def torch_eval(s, d, t, y, T, alpha, mode, lam=1.0, eps=0.0, pair_flip=False, dtype=torch.float64):
    """The reference expression in torch (``dtype``) with autograd's gradients -> dict of ``QUANTITIES`` as numpy fp64."""
    s, d = (v.to(dtype).clone().requires_grad_(True) for v in (s, d))
    t = t.to(dtype)
    B, C = s.shape
    if (lam, eps, pair_flip) == (1.0, 0.0, False):
        ce = TF.cross_entropy(s, y)
    else:
        hot = TF.one_hot(y, C).to(dtype)
        smooth = eps / C + (1.0 - eps) * hot
        ce = TF.cross_entropy(s, lam * smooth + (1.0 - lam) * smooth.flip(0) if pair_flip else smooth)
    if mode == "soft":
        kd = TF.kl_div(TF.log_softmax(d / T, dim=-1), TF.softmax(t / T, dim=-1).detach(), reduction="batchmean") * T ** 2
    else:
        kd = TF.cross_entropy(d, t.argmax(dim=1))
    loss = ce * alpha + kd * (1 - alpha)
    loss.backward()
    n = lambda v: v.detach().double().numpy()
    zeros = np.zeros((B, C))
    return dict(loss=n(loss), ce=n(ce), kd=n(kd), dstudent=n(s.grad) if s.grad is not None else zeros,
                ddistill=n(d.grad) if d.grad is not None else zeros)


def rel_err(got, ref):
    """max|got - ref| / max|ref|; an all-zero reference (a gradient whose weight is 0) asks for all zeros: max|got|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())


@functools.lru_cache(maxsize=None)
def case_oracle(B, C, T, alpha, mode, labelling):
    s, d, t, y = inputs(B, C)
    return oracle(s.numpy(), d.numpy(), t.numpy(), y.numpy(), T, alpha, mode, *labelling)


@functools.lru_cache(maxsize=None)
def baselines():
    """-> {quantity: largest error of torch's fp32 evaluation against the fp64 oracle over every case}: computed once per session."""
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for B, C in itertools.product(BATCHES, CLASSES):
        s, d, t, y = inputs(B, C)
        for T, alpha, mode, labelling in settings():
            ref = case_oracle(B, C, T, alpha, mode, labelling)
            got = torch_eval(s, d, t, y, T, alpha, mode, *labelling, dtype=torch.float32)
            for k in QUANTITIES:
                worst[k] = max(worst[k], rel_err(got[k], ref[k]))
    return worst


def kernel_errors(B, C, device="cuda"):
    """-> {quantity: the kernel's largest error against the oracle over the settings of one (B, C)} (needs the device)."""
    from myrtle_vision.hip import ops
    s, d, t, y = (v.to(device) for v in inputs(B, C))
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for T, alpha, mode, labelling in settings():
        lam, eps, pair_flip = labelling
        ref = case_oracle(B, C, T, alpha, mode, labelling)
        loss, ds, dd, _, _ = ops.distill_loss(s, d, t, y, T, alpha, mode, lam, eps, pair_flip, want_grad=True)
        loss = loss.cpu().double().numpy()
        got = dict(loss=loss[0], ce=loss[1], kd=loss[2], dstudent=ds.cpu().numpy(), ddistill=dd.cpu().numpy())
        for k in QUANTITIES:
            worst[k] = max(worst[k], rel_err(got[k], ref[k]))
    return worst


def main():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "myrtle-vision_amd")]
    base = baselines()
    worst = dict.fromkeys(QUANTITIES, 0.0)
    for B, C in itertools.product(BATCHES, CLASSES):
        for k, v in kernel_errors(B, C).items():
            worst[k] = max(worst[k], v)
    cases = len(BATCHES) * len(CLASSES) * len(settings())
    print("# mv_distill_loss: tolerance table of tests/test_distill_gpu.py, computed when the tests run (nothing is fixed in advance).")
    print(f"# {cases} cases: B in {BATCHES}, C in {CLASSES}, T in {TEMPERATURES}, alpha in {ALPHAS}, {MODES}, plain and")
    print("# (lam 0.3, eps 0.1, pair_flip) labels.  baseline = max over the cases of max|fp32 - fp64| / max|fp64| for torch's own fp32")
    print("# evaluation (CPU) of F.cross_entropy + T^2 * F.kl_div(..., 'batchmean') and autograd's gradients against the fp64 oracle")
    print(f"# (tests/distill_ref.py); bound = {FACTOR:g} x baseline; kernel = the same figure for mv_distill_loss on an MI355X.")
    print("# Regenerate: python tests/distill_ref.py")
    print("# quantity baseline bound kernel")
    for k in QUANTITIES:
        print(f"{k} {base[k]:.6e} {FACTOR * base[k]:.6e} {worst[k]:.6e}")
    return 0 if all(worst[k] <= FACTOR * base[k] for k in QUANTITIES) else 1


if __name__ == "__main__":
    raise SystemExit(main())
