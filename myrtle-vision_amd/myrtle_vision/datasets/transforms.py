"""torchvision-free transforms driven by the reference's JSON ``transform_ops_*`` sections.

Same operations and parameters as the reference builds from torchvision (datasets/resisc45.py:40-69,
datasets/dlrsd.py:39-66, transforms/segmentation.py): Resize((s, s)) bilinear (NEAREST for masks),
RandomResizedCrop(s) with scale (0.08, 1) and ratio (3/4, 4/3), CenterCrop, RandomHorizontalFlip(p=0.5), ToTensor,
Normalize.  Every op takes and returns ``(image, mask_or_None)`` so classification and segmentation share one
pipeline; geometric ops apply the same parameters to both.
"""
import math
import random

import numpy as np
import torch
from PIL import Image

_BILINEAR = Image.Resampling.BILINEAR
_NEAREST = Image.Resampling.NEAREST


class Resize:
    def __init__(self, size):
        self.size = (size, size)

    def __call__(self, img, mask=None):
        return img.resize(self.size, _BILINEAR), (mask.resize(self.size, _NEAREST) if mask is not None else None)


class RandomResizedCrop:
    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
        self.size, self.scale, self.ratio = (size, size), scale, ratio

    def _params(self, w, h):
        area = w * h
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target = area * random.uniform(*self.scale)
            ar = math.exp(random.uniform(*log_ratio))
            cw, ch = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < cw <= w and 0 < ch <= h:
                return random.randint(0, h - ch), random.randint(0, w - cw), ch, cw
        in_ratio = w / h                                     # fallback: central crop at the nearest allowed ratio
        if in_ratio < self.ratio[0]:
            cw, ch = w, int(round(w / self.ratio[0]))
        elif in_ratio > self.ratio[1]:
            ch, cw = h, int(round(h * self.ratio[1]))
        else:
            cw, ch = w, h
        return (h - ch) // 2, (w - cw) // 2, ch, cw

    def __call__(self, img, mask=None):
        top, left, ch, cw = self._params(*img.size)
        box = (left, top, left + cw, top + ch)
        # torchvision F.resized_crop: crop, THEN resize (the filter support clamps at the crop edge; PIL's resize(box=)
        # would reach outside the box)
        img = img.crop(box).resize(self.size, _BILINEAR)
        if mask is not None:
            mask = mask.crop(box).resize(self.size, _NEAREST)
        return img, mask


class CenterCrop:
    def __init__(self, size):
        self.size = size

    def __call__(self, img, mask=None):
        w, h = img.size
        left, top = (w - self.size) // 2, (h - self.size) // 2
        box = (left, top, left + self.size, top + self.size)
        return img.crop(box), (mask.crop(box) if mask is not None else None)


class RandomHorizontalFlip:
    def __call__(self, img, mask=None):
        if random.random() < 0.5:
            img = img.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
            if mask is not None:
                mask = mask.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
        return img, mask


# ---- RandAugment: timm's increasing op set (timm.data.auto_augment, `rand-m9-mstd0.5-inc1`), restated -------------------------
# An extension: the reference augments with crop and flip only.  The op set, the argument of every op and the position in the
# chain are timm's; the order and source of the random draws are this project's own (python's ``random`` only, so that a worker
# needs no numpy seeding).  Pillow calls only: this class is the reference that the device chain (device_transforms.DevicePlan
# + csrc/randaug.hip) is held to, bit for bit.
_BICUBIC = Image.Resampling.BICUBIC
RANDAUG_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd",
               "ColorIncreasing", "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY",
               "TranslateXRel", "TranslateYRel")                  # a slot's code is index + 1; 0 = the slot is skipped
RANDAUG_DEFAULTS = {"magnitude": 9, "magnitude_std": 0.5, "num_ops": 2, "prob": 0.5, "interpolation": "bicubic"}
RANDAUG_GEOMETRIC = frozenset(("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel"))
RANDAUG_ENHANCE = {"ColorIncreasing": "Color", "ContrastIncreasing": "Contrast", "BrightnessIncreasing": "Brightness",
                   "SharpnessIncreasing": "Sharpness"}
_RANDAUG_SIGNED = RANDAUG_GEOMETRIC | frozenset(RANDAUG_ENHANCE)


def randaug_config(config):
    """The ``"RandAugment"`` value of a ``transform_ops_*`` section -> the full parameter dict; ValueError naming what is wrong."""
    config = {} if config is None else config
    if not isinstance(config, dict):
        raise ValueError(f"RandAugment: a dict of {sorted(RANDAUG_DEFAULTS)} expected, got {config!r}")
    unknown = sorted(set(config) - set(RANDAUG_DEFAULTS))
    if unknown:
        raise ValueError(f"RandAugment: unknown key {unknown[0]!r} (known: {sorted(RANDAUG_DEFAULTS)})")
    p = dict(RANDAUG_DEFAULTS, **config)
    number = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool) and v == v
    if not number(p["magnitude"]) or not 0 <= p["magnitude"] <= 10:
        raise ValueError(f"RandAugment: magnitude must be a number in [0, 10], got {p['magnitude']!r}")
    if not number(p["magnitude_std"]) or not 0 <= p["magnitude_std"] < math.inf:
        raise ValueError(f"RandAugment: magnitude_std must be a number >= 0, got {p['magnitude_std']!r}")
    if not isinstance(p["num_ops"], int) or isinstance(p["num_ops"], bool) or p["num_ops"] < 1:
        raise ValueError(f"RandAugment: num_ops must be an integer >= 1, got {p['num_ops']!r}")
    if not number(p["prob"]) or not 0 <= p["prob"] <= 1:
        raise ValueError(f"RandAugment: prob must be a number in [0, 1], got {p['prob']!r}")
    if p["interpolation"] not in ("bilinear", "bicubic", "random"):
        raise ValueError(f"RandAugment: interpolation must be 'bilinear', 'bicubic' or 'random', got {p['interpolation']!r}")
    return p


def randaug_argument(name, level, negate, width, height):
    """The argument of op ``name`` at ``level`` in [0, 1] (timm's ``_*_level_to_arg``): degrees, shear factor, translation in pixels,
    bits, threshold, addend, enhance factor; None for the three ops without one."""
    sign = -1.0 if negate else 1.0
    if name == "Rotate":
        return sign * (30.0 * level)
    if name in ("ShearX", "ShearY"):
        return sign * (0.3 * level)
    if name == "TranslateXRel":
        return sign * (0.45 * level) * width
    if name == "TranslateYRel":
        return sign * (0.45 * level) * height
    if name == "PosterizeIncreasing":
        return 4 - int(4 * level)
    if name == "SolarizeIncreasing":
        return 256 - int(256 * level)
    if name == "SolarizeAdd":
        return min(128, int(110 * level))
    if name in RANDAUG_ENHANCE:
        return max(0.1, 1.0 + sign * (0.9 * level))
    return None


def rotate_matrix(degrees, width, height):
    """The six AFFINE coefficients ``Image.rotate(degrees)`` hands to ``Image.transform`` (expand=False, centre of the image)."""
    angle = -math.radians(degrees % 360.0)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    cx, cy = width / 2, height / 2
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def affine_coefficients(name, arg, width, height):
    """Geometric op -> the coefficients of ``Image.transform(size, AFFINE, .)``."""
    if name == "Rotate":
        return rotate_matrix(arg, width, height)
    return {"ShearX": (1, arg, 0, 0, 1, 0), "ShearY": (1, 0, 0, arg, 1, 0), "TranslateXRel": (1, 0, arg, 0, 1, 0),
            "TranslateYRel": (1, 0, 0, 0, 1, arg)}[name]


class RandAugment:
    """``num_ops`` slots per image, each an op of ``RANDAUG_OPS`` drawn with replacement and applied with probability ``prob`` at a
    magnitude drawn round ``magnitude`` (of 10).  ``fill``: the colour a geometric op leaves outside the source."""

    def __init__(self, config=None, mean=None):
        p = randaug_config(config)
        self.magnitude, self.magnitude_std, self.num_ops = float(p["magnitude"]), float(p["magnitude_std"]), p["num_ops"]
        self.prob, self.interpolation = float(p["prob"]), p["interpolation"]
        self.fill = (128, 128, 128) if mean is None else tuple(min(255, round(255 * float(m))) for m in mean)
        if len(self.fill) != 3 or min(self.fill) < 0:
            raise ValueError(f"RandAugment: the fill colour comes from a 3-channel Normalize mean in [0, 1], got {mean!r}")
        self.applied = None                               # the slots of the last call, as ``draw`` returned them

    def draw(self, width, height):
        """Every random draw of one image -> per slot None (skipped) or (name, argument, resample | None)."""
        names = [RANDAUG_OPS[random.randrange(len(RANDAUG_OPS))] for _ in range(self.num_ops)]
        slots = []
        for name in names:
            if random.random() > self.prob:
                slots.append(None)
                continue
            m = random.gauss(self.magnitude, self.magnitude_std) if self.magnitude_std > 0 else self.magnitude
            level = min(10.0, max(0.0, m)) / 10
            negate = name in _RANDAUG_SIGNED and random.random() > 0.5
            resample = None
            if name in RANDAUG_GEOMETRIC:
                resample = {"bilinear": _BILINEAR, "bicubic": _BICUBIC}.get(self.interpolation)
                if resample is None:
                    resample = random.choice((_BILINEAR, _BICUBIC))
            slots.append((name, randaug_argument(name, level, negate, width, height), resample))
        return slots

    def apply_op(self, img, name, arg, resample):
        from PIL import ImageEnhance, ImageOps
        if name == "Rotate":
            return img.rotate(arg, resample, fillcolor=self.fill)
        if name in RANDAUG_GEOMETRIC:
            coeffs = affine_coefficients(name, arg, *img.size)
            return img.transform(img.size, Image.Transform.AFFINE, coeffs, resample, fillcolor=self.fill)
        if name in RANDAUG_ENHANCE:
            return getattr(ImageEnhance, RANDAUG_ENHANCE[name])(img).enhance(arg)
        if name == "PosterizeIncreasing":
            return ImageOps.posterize(img, arg)
        if name == "SolarizeIncreasing":
            return ImageOps.solarize(img, arg)
        if name == "SolarizeAdd":
            lut = [min(255, i + arg) if i < 128 else i for i in range(256)]
            return img.point(lut * 3)
        return {"AutoContrast": ImageOps.autocontrast, "Equalize": ImageOps.equalize, "Invert": ImageOps.invert}[name](img)

    def __call__(self, img, mask=None):
        if mask is not None:
            raise ValueError("RandAugment is for classification: geometric ops on a label map are not supported")
        img = img.convert("RGB")
        self.applied = self.draw(*img.size)
        for slot in self.applied:
            if slot is not None:
                img = self.apply_op(img, *slot)
        return img, None


class ToTensorNormalize:
    """ToTensor (HWC uint8 -> CHW float in [0,1]) followed by the optional Normalize(mean, std)."""

    def __init__(self, mean=None, std=None):
        self.mean = None if mean is None else torch.tensor(mean, dtype=torch.float32).view(-1, 1, 1)
        self.std = None if std is None else torch.tensor(std, dtype=torch.float32).view(-1, 1, 1)

    def __call__(self, img, mask=None):
        a = np.asarray(img.convert("RGB"), dtype=np.uint8)
        t = torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0)
        if self.mean is not None:
            t = (t - self.mean) / self.std
        if mask is not None:
            mask = torch.from_numpy(np.asarray(mask, dtype=np.uint8).copy()).to(torch.int64)
        return t, mask


class Compose:
    def __init__(self, ops):
        self.ops = ops

    def __call__(self, img, mask=None):
        for op in self.ops:
            img, mask = op(img, mask)
        return img, mask


def build_transform(transform_config):
    """Order of the reference: Resize, RandomResizedCrop, CenterCrop, RandomHorizontalFlip, ToTensor, Normalize."""
    ops = []
    if "Resize" in transform_config:
        ops.append(Resize(transform_config["Resize"]))
    if "RandomResizedCrop" in transform_config:
        ops.append(RandomResizedCrop(transform_config["RandomResizedCrop"]))
    if "CenterCrop" in transform_config:
        ops.append(CenterCrop(transform_config["CenterCrop"]))
    if "RandomHorizontalFlip" in transform_config:
        ops.append(RandomHorizontalFlip())
    n = transform_config.get("Normalize")
    if "RandAugment" in transform_config:                    # timm's position: after the geometry, before ToTensor
        ops.append(RandAugment(transform_config["RandAugment"], n["Mean"] if n else None))
    ops.append(ToTensorNormalize(n["Mean"], n["Std"]) if n else ToTensorNormalize())
    return Compose(ops)
