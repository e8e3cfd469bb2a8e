"""Detection transforms on (image, target) pairs and the padded-batch collate, torchvision-free.

Counterpart of the reference's ``src/myrtle_vision/transforms/detection.py`` (the DETR transforms with the YOLOS size rule):
the same operations, the same random draws in the same order, the same fp32 box arithmetic, so a seeded run follows the
reference sample for sample.  ``target`` is the dict ``datasets/coco.py`` builds: ``boxes`` xyxy fp32 [T, 4] in pixels of the
current image, ``labels``, ``area``, ``iscrowd`` [T], ``size`` / ``orig_size`` = (h, w).

Every geometric op touches the image through four members only -- ``size`` / ``width`` / ``height``, ``crop(box)``,
``transpose(FLIP_LEFT_RIGHT)`` and ``resize((w, h), BILINEAR)`` -- so the chain runs unchanged on a PIL image (host path) and
on ``device_transforms.TableFrame``, which records the same geometry as resampling tables for the GPU (device path).  The box
arithmetic is therefore literally shared between the two paths.

Random draws: ``random.random`` (flip, select), ``random.choice`` (resize scale), ``random.randint`` (crop size), and for the
crop OFFSET ``torch.randint`` twice (top, then left) -- the reference takes the offset from torchvision's
``RandomCrop.get_params``, which draws from torch's generator and draws nothing when the crop is the whole image.
"""
import random

import numpy as np
import torch
from PIL import Image

_BILINEAR = Image.Resampling.BILINEAR
_FLIP = Image.Transpose.FLIP_LEFT_RIGHT
_PER_BOX = ("labels", "area", "iscrowd", "boxes")


# ---- the padded batch ---------------------------------------------------------------------------------------------
class NestedTensor:
    """``tensors`` [B, C, Hmax, Wmax], zero outside every image's own extent, and ``mask`` bool [B, Hmax, Wmax], True there."""

    def __init__(self, tensors, mask):
        self.tensors, self.mask = tensors, mask

    def to(self, device):
        return NestedTensor(self.tensors.to(device), None if self.mask is None else self.mask.to(device))

    def decompose(self):
        return self.tensors, self.mask

    def __repr__(self):
        return str(self.tensors)


def nested_tensor_from_tensor_list(tensor_list):
    if tensor_list[0].ndim != 3:
        raise ValueError("not supported")
    c, h, w = (max(t.shape[d] for t in tensor_list) for d in range(3))
    batch = torch.zeros((len(tensor_list), c, h, w), dtype=tensor_list[0].dtype, device=tensor_list[0].device)
    mask = torch.ones((len(tensor_list), h, w), dtype=torch.bool, device=tensor_list[0].device)
    for i, t in enumerate(tensor_list):
        batch[i, :t.shape[0], :t.shape[1], :t.shape[2]] = t
        mask[i, :t.shape[1], :t.shape[2]] = False
    return NestedTensor(batch, mask)


def collate_fn(batch):
    """[(image, target), ...] -> (NestedTensor of the images, tuple of the targets)."""
    images, targets = zip(*batch)
    return nested_tensor_from_tensor_list(list(images)), tuple(targets)


# ---- geometry + target arithmetic ------------------------------------------------------------------------------------
def crop(image, target, region):
    """``region`` = (top, left, height, width).  Boxes are shifted, clamped to the window and dropped when nothing is left."""
    top, left, h, w = region
    image = image.crop((left, top, left + w, top + h))
    target = dict(target)
    target["size"] = torch.tensor([h, w])
    if "boxes" in target:
        corners = target["boxes"] - torch.as_tensor([left, top, left, top])
        corners = torch.min(corners.reshape(-1, 2, 2), torch.as_tensor([w, h], dtype=torch.float32)).clamp(min=0)
        target["area"] = (corners[:, 1, :] - corners[:, 0, :]).prod(dim=1)
        target["boxes"] = corners.reshape(-1, 4)
        keep = torch.all(corners[:, 1, :] > corners[:, 0, :], dim=1)
        for field in _PER_BOX:
            target[field] = target[field][keep]
    return image, target


def hflip(image, target):
    w, _ = image.size
    image = image.transpose(_FLIP)
    target = dict(target)
    if "boxes" in target:
        target["boxes"] = target["boxes"][:, [2, 1, 0, 3]] * torch.as_tensor([-1, 1, -1, 1]) + torch.as_tensor([w, 0, w, 0])
    return image, target


def output_size(image_size, size, max_size=None):
    """(w, h) of the image and the requested short side -> (oh, ow): the short side becomes ``size`` -- lowered first so that
    the long side stays within ``max_size`` --, the long side follows the aspect ratio (truncated), and both are floored to a
    multiple of 16 (the patch size).  An image whose short side already equals ``size`` keeps its sides, floored alike."""
    if isinstance(size, (list, tuple)):
        return tuple(size[::-1])
    w, h = image_size
    if max_size is not None:
        short, long = float(min(w, h)), float(max(w, h))
        if long / short * size > max_size:
            size = int(round(max_size * short / long))
    if (w <= h and w == size) or (h <= w and h == size):
        oh, ow = h, w
    elif w < h:
        oh, ow = int(size * h / w), size
    else:
        oh, ow = size, int(size * w / h)
    return int(oh - oh % 16), int(ow - ow % 16)


def resize(image, target, size, max_size=None):
    oh, ow = output_size(image.size, size, max_size)
    w0, h0 = image.size
    image = image.resize((ow, oh), _BILINEAR)
    if target is None:
        return image, None
    rw, rh = float(ow) / float(w0), float(oh) / float(h0)
    target = dict(target)
    if "boxes" in target:
        target["boxes"] = target["boxes"] * torch.as_tensor([rw, rh, rw, rh])
    if "area" in target:
        target["area"] = target["area"] * (rw * rh)
    target["size"] = torch.tensor([oh, ow])
    return image, target


def crop_offset(h, w, th, tw):
    """Top-left corner of a (th, tw) window in an (h, w) image: nothing is drawn when the window is the image, else top and
    left come from torch's generator, in that order."""
    if h < th or w < tw:
        raise ValueError(f"crop {(th, tw)} larger than the image {(h, w)}")
    if h == th and w == tw:
        return 0, 0
    top = int(torch.randint(0, h - th + 1, size=(1,)).item())
    left = int(torch.randint(0, w - tw + 1, size=(1,)).item())
    return top, left


# ---- the transform classes -----------------------------------------------------------------------------------------------
class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, img, target):
        if random.random() < self.p:
            return hflip(img, target)
        return img, target


class RandomResize:
    def __init__(self, sizes, max_size=None):
        assert isinstance(sizes, (list, tuple))
        self.sizes, self.max_size = sizes, max_size

    def __call__(self, img, target=None):
        return resize(img, target, random.choice(self.sizes), self.max_size)


class RandomSizeCrop:
    def __init__(self, min_size, max_size):
        self.min_size, self.max_size = min_size, max_size

    def __call__(self, img, target):
        w = random.randint(self.min_size, min(img.width, self.max_size))
        h = random.randint(self.min_size, min(img.height, self.max_size))
        top, left = crop_offset(img.height, img.width, h, w)
        return crop(img, target, (top, left, h, w))


class RandomSelect:
    """``first`` with probability p, else ``second``."""

    def __init__(self, first, second, p=0.5):
        self.first, self.second, self.p = first, second, p

    def __call__(self, img, target):
        if random.random() < self.p:
            return self.first(img, target)
        return self.second(img, target)


class ToTensor:
    """PIL image -> fp32 [3, h, w] in [0, 1].  A table frame (device path) passes through: the kernel does this step."""

    def __call__(self, img, target):
        if not isinstance(img, Image.Image):
            return img, target
        a = np.asarray(img.convert("RGB"), dtype=np.uint8)
        return torch.from_numpy(a.copy()).permute(2, 0, 1).float().div_(255.0), target


class Normalize:
    """(x - mean) / std per channel; boxes become (cx, cy, w, h) divided by the image's (w, h, w, h)."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, std

    def __call__(self, image, target=None):
        if torch.is_tensor(image):
            mean = torch.tensor(self.mean, dtype=torch.float32).view(-1, 1, 1)
            std = torch.tensor(self.std, dtype=torch.float32).view(-1, 1, 1)
            image = (image - mean) / std
            h, w = image.shape[-2:]
        else:                                                  # table frame: the kernel normalises
            image = image.normalized(self.mean, self.std)
            h, w = image.height, image.width
        if target is None:
            return image, None
        target = dict(target)
        if "boxes" in target:
            x0, y0, x1, y1 = target["boxes"].unbind(-1)
            boxes = torch.stack(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0), dim=-1)
            target["boxes"] = boxes / torch.tensor([w, h, w, h], dtype=torch.float32)
        return image, target


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        for t in self.transforms:
            image, target = t(image, target)
        return image, target

    def __repr__(self):
        return "Compose(" + ", ".join(type(t).__name__ for t in self.transforms) + ")"


def _ops_from_config(section):
    ops = []
    for key, value in section.items():                         # JSON object order IS the chain order
        if key == "RandomHorizontalFlip":
            ops.append(RandomHorizontalFlip())
        elif key.endswith("RandomResize"):                     # RandomResize, PreRandomResize, PostRandomResize
            scales, ratio = value["scales"], value.get("max_size_ratio")
            ops.append(RandomResize(scales, max_size=None if ratio is None else max(scales) * ratio[0] // ratio[1]))
        elif key == "RandomSizeCrop":
            ops.append(RandomSizeCrop(value[0], value[1]))
        elif key == "RandomSelect":
            first, second = _ops_from_config(value)
            ops.append(RandomSelect(first, second))
        elif key == "Normalize":
            ops += [ToTensor(), Normalize(mean=value["Mean"], std=value["Std"])]
        elif key == "Compose":
            ops.append(Compose(_ops_from_config(value)))
        # anything else (RandomErasing, RandomPad, CenterCrop ...) is ignored, as by the reference
    return ops


def from_config(transform_config):
    """A ``transform_ops_train`` / ``transform_ops_val`` section of the detection data config -> the transform chain."""
    return Compose(_ops_from_config(transform_config))
