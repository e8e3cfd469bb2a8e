"""Mixup and CutMix of a device batch, in place, on the HIP kernel (``mv_mix_batch``).

A restatement of timm's ``timm.data.Mixup`` in batch mode: one ``lam`` (and one box) per batch, sample ``i`` paired with sample
``B - 1 - i`` (timm's ``x.flip(0)``).  timm is not available offline and the reference never mixes, so the ORDER AND SOURCE of the
random draws are a restatement too (PARITY UNPINNED, as ``utils/optim.py`` says of its schedule): timm draws from ``numpy.random``,
this class from Python's ``random``, which ``seed_everything`` seeds and the host transforms already use.  Per batch:

1. with probability ``prob`` the batch is mixed, else ``lam = 1`` and nothing is launched;
2. with both alphas > 0, CutMix is chosen with probability ``switch_prob``; with one alpha > 0, that mode;
3. ``lam ~ Beta(alpha, alpha)`` of the chosen mode;
4. CutMix: ``r = sqrt(1 - lam)``, ``cut_h = int(H * r)``, ``cut_w = int(W * r)``, the centre uniform over the image's pixels, the
   edges ``clip(centre -/+ cut // 2, 0, size)``; then ``lam = 1 - box_area / (H * W)``, the share of the image that stayed.

The labels are not touched: the soft target is formed inside the loss kernel (``hip.functional.SoftTargetCrossEntropy``) from the
hard labels, the same pairing and ``lam``.
"""
import math
import random

MIXUP, CUTMIX = 0, 1


class Mixup:
    """``mixer(imgs, labels) -> (imgs, lam)``: mixes the [B, Ch, H, W] device batch IN PLACE and returns the ``lam`` to hand to the
    criterion.  ``lam`` and the box are host scalars that become launch arguments: there is no device-to-host copy and no
    synchronisation -- and for the same reason a captured step (``utils/graph.py``) cannot contain a ``Mixup``: a replay would
    repeat the scalars of the capture."""

    def __init__(self, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0, switch_prob=0.5):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("mixup_alpha and cutmix_alpha must be >= 0")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("prob and switch_prob are probabilities")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)

    @property
    def enabled(self):
        return self.mixup_alpha > 0 or self.cutmix_alpha > 0

    def params(self, H, W):
        """One batch's draw, on the host: ``(mode, lam, box)`` with ``mode`` MIXUP (0) or CUTMIX (1) and ``box`` =
        ``(y0, y1, x0, x1)`` for CutMix, else None.  An unmixed batch is ``(MIXUP, 1.0, None)``."""
        if not self.enabled or random.random() >= self.prob:
            return MIXUP, 1.0, None
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = random.random() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        if not cut:
            return MIXUP, random.betavariate(self.mixup_alpha, self.mixup_alpha), None
        lam = random.betavariate(self.cutmix_alpha, self.cutmix_alpha)
        r = math.sqrt(1.0 - lam)
        cut_h, cut_w = int(H * r), int(W * r)
        cy, cx = random.randrange(H), random.randrange(W)
        clip = lambda v, hi: min(max(v, 0), hi)
        y0, y1 = clip(cy - cut_h // 2, H), clip(cy + cut_h // 2, H)
        x0, x1 = clip(cx - cut_w // 2, W), clip(cx + cut_w // 2, W)
        return CUTMIX, 1.0 - (y1 - y0) * (x1 - x0) / (H * W), (y0, y1, x0, x1)

    def __call__(self, imgs, labels):
        from myrtle_vision.hip import ops
        if not imgs.is_contiguous():
            imgs = imgs.contiguous()             # the kernel walks a dense batch; the caller goes on with the returned tensor
        mode, lam, box = self.params(imgs.shape[-2], imgs.shape[-1])
        if mode == CUTMIX:
            ops.mix_batch(imgs, box=box)
        elif lam != 1.0:
            ops.mix_batch(imgs, lam=lam)
        return imgs, lam
