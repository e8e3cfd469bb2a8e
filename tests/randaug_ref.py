"""What the RandAugment tests share: the direct Pillow call of every op (written here from timm's auto_augment.py and Pillow's
documentation, not imported from the package), the test images, the per-op parameter cases, and the host build of
csrc/randaug_math.h."""
import ctypes
import os
import subprocess

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIL, BIC = Image.Resampling.BILINEAR, Image.Resampling.BICUBIC
OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
       "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
GEOMETRIC = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
ENHANCE = {"ColorIncreasing": ImageEnhance.Color, "ContrastIncreasing": ImageEnhance.Contrast,
           "BrightnessIncreasing": ImageEnhance.Brightness, "SharpnessIncreasing": ImageEnhance.Sharpness}
FILL = (124, 116, 104)                    # round(255 * ImageNet mean)
SIZES = [(1, 1), (2, 5), (3, 3), (37, 53), (224, 224)]


def pillow_op(img, name, arg=None, resample=None, fill=FILL):
    """PIL image -> PIL image: op ``name`` of timm's increasing set with its argument (degrees / shear factor / pixels / bits /
    threshold / addend / enhance factor)."""
    w, h = img.size
    affine = lambda m: img.transform((w, h), Image.Transform.AFFINE, m, resample, fillcolor=fill)
    if name == "Rotate":
        return img.rotate(arg, resample, fillcolor=fill)
    if name == "ShearX":
        return affine((1, arg, 0, 0, 1, 0))
    if name == "ShearY":
        return affine((1, 0, 0, arg, 1, 0))
    if name == "TranslateXRel":
        return affine((1, 0, arg, 0, 1, 0))
    if name == "TranslateYRel":
        return affine((1, 0, 0, 0, 1, arg))
    if name in ENHANCE:
        return ENHANCE[name](img).enhance(arg)
    if name == "PosterizeIncreasing":
        return ImageOps.posterize(img, arg)
    if name == "SolarizeIncreasing":
        return ImageOps.solarize(img, arg)
    if name == "SolarizeAdd":
        return img.point([min(255, i + arg) if i < 128 else i for i in range(256)] * 3)
    return {"AutoContrast": ImageOps.autocontrast, "Equalize": ImageOps.equalize, "Invert": ImageOps.invert}[name](img)


def images(h, w, seed=0):
    """The five test images, uint8 [h, w, 3]: uniform noise, flat, two-level, horizontal ramp, noise limited to [40, 200)."""
    rng = np.random.default_rng(seed * 7919 + h * 1000 + w)
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flat = np.broadcast_to(np.array([37, 150, 222], np.uint8), (h, w, 3)).copy()
    two = np.where(rng.random((h, w, 1)) < 0.5, np.uint8(30), np.uint8(201)) + np.zeros((1, 1, 3), np.uint8)
    ramp = np.broadcast_to((np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8)[None, :, None], (h, w, 3)).copy()
    ramp[..., 1] = 255 - ramp[..., 1]
    limited = rng.integers(40, 200, (h, w, 3), dtype=np.uint8)
    return [noise, flat, two.astype(np.uint8), ramp, limited]


def autocontrast_images():
    """255 images of 16 x 16, one for each hi - lo in 1..255, lo varied (per channel) over what fits; every level from lo to hi is
    present.  Where hi - lo does not divide 255 the table's products sit next to integers: a contracted or inexactly divided
    table truncates differently."""
    rng = np.random.default_rng(255)
    out = []
    for d in range(1, 256):
        a = np.empty((256, 3), np.uint8)
        for c in range(3):
            lo = (d * 11 + c * 37) % (256 - d)
            a[:, c] = rng.permutation(np.resize(np.arange(lo, lo + d + 1), 256))
        out.append(a.reshape(16, 16, 3))
    return out


class Guarded:
    """Integer tensors between sentinel zones (GUARD elements of the tensor's dtype on each side, value 0x5A): ``new`` gives the
    view, ``check`` asserts that no kernel wrote outside."""
    GUARD, SENTINEL = 256, 0x5A

    def __init__(self, torch, device="cuda"):
        self.torch, self.device, self.zones = torch, device, []

    def new(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        buf = self.torch.full((n + 2 * self.GUARD,), self.SENTINEL, dtype=dtype, device=self.device)
        view = buf[self.GUARD:self.GUARD + n].view(*shape)
        if fill is not None:
            view.copy_(fill)
        self.zones.append(buf)
        return view

    def check(self):
        g = self.GUARD
        for buf in self.zones:
            assert bool((buf[:g] == self.SENTINEL).all()) and bool((buf[-g:] == self.SENTINEL).all()), "a kernel wrote outside its tensor"


def op_cases(h, w):
    """(name, argument, resample) for every op: both signs and both ends of each range."""
    cases = [("AutoContrast", None, None), ("Equalize", None, None), ("Invert", None, None)]
    for r in (BIL, BIC):
        cases += [("Rotate", d, r) for d in (0.0, 30.0, -30.0, 13.7)]
        cases += [(n, f, r) for n in ("ShearX", "ShearY") for f in (0.3, -0.3, 0.0, 0.1234)]
        cases += [("TranslateXRel", s * 0.45 * w, r) for s in (1, -1)] + [("TranslateXRel", 0.1 * w + 0.3, r)]
        cases += [("TranslateYRel", s * 0.45 * h, r) for s in (1, -1)] + [("TranslateYRel", -0.2 * h - 0.6, r)]
    cases += [("PosterizeIncreasing", b, None) for b in (0, 1, 4)]
    cases += [("SolarizeIncreasing", t, None) for t in (0, 100, 256)]
    cases += [("SolarizeAdd", a, None) for a in (0, 57, 110)]
    cases += [(n, f, None) for n in ENHANCE for f in (0.1, 0.5, 1.0, 1.9)]
    return cases


def fields(slots, w, h):
    """[(name, arg, resample) | None, ...] of ONE sample -> (ra_op int32 [n], ra_par float64 [n, 8]), by the package's packer."""
    from myrtle_vision.datasets.device_transforms import DevicePlan
    return DevicePlan.randaug_fields(slots, w, h)


# ---- csrc/randaug_math.h on the host --------------------------------------------------------------------------------------------
def host_library(directory):
    """Compile tests/randaug_host.cpp (csrc/randaug_math.h for the host) into ``directory`` and bind it."""
    so = os.path.join(str(directory), "randaug_host.so")
    cmd = ["g++", "-O2", "-shared", "-fPIC", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "myrtle-vision_amd", "csrc"),
           os.path.join(ROOT, "tests", "randaug_host.cpp"), "-o", so]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = ctypes.CDLL(so)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.ra_host_affine.argtypes = [P, I, I, P, I, P, P]
    lib.ra_host_enhance.argtypes = [P, I, I, I, ctypes.c_double, P]
    lib.ra_host_table.argtypes = [P, I, I, I, I, P]
    for f in (lib.ra_host_affine, lib.ra_host_enhance, lib.ra_host_table):
        f.restype = None
    return lib


def host_op(lib, a, name, arg, resample, fill=FILL):
    """uint8 [h, w, 3] -> uint8 [h, w, 3] through the host build, fed with the fields the device would get."""
    a = np.ascontiguousarray(a)
    h, w = a.shape[:2]
    op, par = fields([(name, arg, resample)], w, h)
    out = np.empty_like(a)
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    if name in GEOMETRIC:
        coeffs, fl = np.ascontiguousarray(par[0, :6]), np.asarray(fill, np.int32)
        lib.ra_host_affine(p(a), h, w, p(coeffs), int(par[0, 6]), p(fl), p(out))
    elif name in ENHANCE:
        lib.ra_host_enhance(p(a), h, w, int(op[0]), float(par[0, 0]), p(out))
    else:
        table = np.empty((3, 256), np.uint8)
        lib.ra_host_table(p(a), h, w, int(op[0]), int(par[0, 0]), p(table))
        out = np.stack([table[c][a[..., c]] for c in range(3)], axis=-1)
    return out
