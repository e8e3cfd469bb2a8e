"""Image preparation split between the DataLoader worker and the GPU.

The reference's workers run the whole torchvision/Pillow chain per image and ship fp32 tensors
(datasets/resisc45.py:40-69, datasets/dlrsd.py:39-66, ``num_workers=1, pin_memory=False``: classification/train.py:117-125).
Here the worker only DECODES the file and draws the random parameters; it hands over

  * the decoded frame as uint8 HWC (3x fewer bytes over PCIe than the fp32 CHW tensor), and
  * per axis, Pillow's resampling tables for that image's crop box (a few KB: ``bilinear_tables``),

and one HIP kernel (``mv_image_prepare``; ``mv_mask_prepare`` for segmentation masks) does crop + antialiased bilinear
resize + flip + ToTensor + Normalize for the whole batch, bit-exact to the Pillow path in ``datasets/transforms.py``
(tests/test_image_prep.py).  Supported chains (all the reference's configs): [Resize] -> [RandomResizedCrop] ->
[CenterCrop] -> [RandomHorizontalFlip] -> ToTensor -> [Normalize].  Resize FOLLOWED BY RandomResizedCrop (the
segmentation training config) is two resamplings, each rounded to uint8 by Pillow: the GPU runs them as two kernels
(``mv_image_resize_u8`` / ``mv_mask_resize_u8`` keep the intermediate uint8 image), with a second set of tables.

With the optional ``"RandAugment"`` key (classification only; timm's increasing op set, ``datasets/transforms.RandAugment``) the
chain is ... -> [RandomHorizontalFlip] -> RandAugment -> ToTensor -> [Normalize]: the worker also draws each slot's op and argument
(``ra_op`` / ``ra_par``) and folds the flip into the last stage's horizontal tables; the GPU keeps the last resampling as uint8
(``mv_image_resize_u8``), runs ``mv_randaug_stats`` + ``mv_randaug_apply`` per slot and finishes with ``mv_image_prepare`` through
copying tables -- bit-exact to the Pillow calls of the host chain (tests/test_randaug_gpu.py).

Detection (``DetectionDevicePlan``) differs in one way: every image leaves its chain with its own size and the batch is the
zero-padded stack of them.  ``mv_image_prepare_ragged`` / ``mv_image_resize_u8_ragged`` take per-sample extents and write the
padding and the padding mask themselves.
"""
import math
import random

import numpy as np
import torch

from myrtle_vision.datasets.transforms import RANDAUG_GEOMETRIC, RANDAUG_OPS, RandAugment, RandomResizedCrop, affine_coefficients

PRECISION_BITS = 22          # Pillow Resample.c: 32 - 8 - 2
MAX_TAPS = 64                # mv_image_prepare's limit on taps per output pixel (downscale factor < ~31)


def bilinear_tables(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BILINEAR over a whole axis of ``in_size`` pixels, vectorised
    over the output pixels with the C code's operation order (IEEE double: identical results).
    -> (bounds int32 [out, 2] = (first source index, tap count), kk int32 [out, ksize])"""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    xmin = np.trunc(center - support + 0.5).astype(np.int64)
    xmin = np.maximum(xmin, 0)
    xmax = np.trunc(center + support + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_size) - xmin
    k = np.arange(ksize, dtype=np.int64)[None, :]
    valid = k < xmax[:, None]
    v = ((k + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss
    v = np.abs(v)
    w = np.where(valid & (v < 1.0), 1.0 - v, 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                   # same left-to-right accumulation as the C loop
        ww = ww + w[:, j]
    w = np.where((ww != 0.0)[:, None], w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    kk[~valid] = 0
    return np.stack([xmin, xmax], axis=1).astype(np.int32), kk


def nearest_table(in_size, out_size):
    """Source index per output pixel of Pillow's NEAREST resize of a whole axis (Geometry.c ImagingScaleAffine:
    ``xo = a0 / 2`` advanced by ``xo += a0`` -- the running sum, not a product), clamped into range."""
    a0 = float(in_size) / out_size
    xo = np.empty(out_size, np.float64)
    acc = 0.0 + a0 * 0.5
    for x in range(out_size):
        xo[x] = acc
        acc += a0
    return np.clip(np.trunc(xo).astype(np.int64), 0, in_size - 1).astype(np.int32)


class DevicePlan:
    """Built from a reference ``transform_ops_*`` section.  ``__call__(pil_image, pil_mask)`` -> one sample dict of
    small CPU tensors (decoded frame + tables); ``collate`` stacks them; ``apply`` runs the kernels on the GPU."""

    def __init__(self, transform_config):
        unknown = set(transform_config) - {"Resize", "RandomResizedCrop", "CenterCrop", "RandomHorizontalFlip", "Normalize",
                                          "RandAugment"}
        if unknown:
            raise ValueError(f"transform chain not supported on the device path: {sorted(transform_config)}")
        self.resize = transform_config.get("Resize")
        self.rrc = RandomResizedCrop(transform_config["RandomResizedCrop"]) if "RandomResizedCrop" in transform_config else None
        self.center = transform_config.get("CenterCrop")
        self.flip = "RandomHorizontalFlip" in transform_config
        n = transform_config.get("Normalize")
        self.mean = tuple(float(v) for v in n["Mean"]) if n else (0.0, 0.0, 0.0)
        self.std = tuple(float(v) for v in n["Std"]) if n else (1.0, 1.0, 1.0)
        # RandAugment (classification only): the host chain's own object makes the draws, so both sides draw alike; a bad
        # value raises here, before any device work
        self.randaug = RandAugment(transform_config["RandAugment"], n["Mean"] if n else None) if "RandAugment" in transform_config else None
        self._cache = {}
        self._identity = {}

    def __getstate__(self):
        return dict(self.__dict__, _identity={})             # device tensors stay in the process that made them

    # ---- worker side ------------------------------------------------------------------------------------------
    def _tables(self, n_in, n_out):
        t = self._cache.get((n_in, n_out))
        if t is None:
            if len(self._cache) > 4096:
                self._cache.clear()
            t = self._cache[(n_in, n_out)] = bilinear_tables(n_in, n_out) + (nearest_table(n_in, n_out),)
        return t

    def __call__(self, img, mask=None):
        a = np.asarray(img.convert("RGB"), dtype=np.uint8)
        H, W = a.shape[:2]
        first = None
        if self.rrc is not None and self.resize is not None:
            # stage one: Resize((S, S)) of the whole frame; the crop below then lives on that S x S uint8 image
            S = int(self.resize)
            b1v, k1v, y1 = self._tables(H, S)
            b1h, k1h, x1 = self._tables(W, S)
            first = (b1v, k1v, y1, b1h, k1h, x1)
            H = W = S
        # same draws, in the same order, as transforms.RandomResizedCrop / RandomHorizontalFlip
        if self.rrc is not None:
            top, left, ch, cw = self.rrc._params(W, H)
            oh = ow = self.rrc.size[0]
        else:
            top, left, ch, cw = 0, 0, H, W
            oh = ow = self.resize if self.resize is not None else None
        if oh is None:
            oh, ow = ch, cw
        bv, kv, yi = self._tables(ch, oh)
        bh, kh, xi = self._tables(cw, ow)
        bv, bh, yi, xi = bv.copy(), bh.copy(), yi + top, xi + left
        bv[:, 0] += top
        bh[:, 0] += left
        if self.center is not None:                          # CenterCrop of the resized image = a window of the tables
            c = int(self.center)
            t0, l0 = (oh - c) // 2, (ow - c) // 2
            bv, kv, yi, bh, kh, xi = bv[t0:t0 + c], kv[t0:t0 + c], yi[t0:t0 + c], bh[l0:l0 + c], kh[l0:l0 + c], xi[l0:l0 + c]
        flip = 1 if (self.flip and random.random() < 0.5) else 0
        ra = None
        if self.randaug is not None:
            if mask is not None:
                raise ValueError("RandAugment is for classification: geometric ops on a label map are not supported")
            if flip:                                         # the flip precedes RandAugment: fold it into the final stage's
                bh, kh, flip = bh[::-1], kh[::-1], 0         # horizontal tables (row order reversed, as TableFrame.transpose does)
            ra = self.randaug_fields(self.randaug.draw(len(bh), len(bv)), len(bh), len(bv))
        s = {"raw": torch.from_numpy(a.copy()), "kh": torch.from_numpy(np.ascontiguousarray(kh)),
             "bh": torch.from_numpy(np.ascontiguousarray(bh)), "kv": torch.from_numpy(np.ascontiguousarray(kv)),
             "bv": torch.from_numpy(np.ascontiguousarray(bv)), "flip": flip}
        if first is not None:
            s.update(kv1=torch.from_numpy(np.ascontiguousarray(first[1])), bv1=torch.from_numpy(np.ascontiguousarray(first[0])),
                     kh1=torch.from_numpy(np.ascontiguousarray(first[4])), bh1=torch.from_numpy(np.ascontiguousarray(first[3])))
        if ra is not None:
            s.update(ra_op=torch.from_numpy(ra[0]), ra_par=torch.from_numpy(ra[1]))
        if mask is not None:
            m = np.asarray(mask, dtype=np.uint8)
            if m.shape != a.shape[:2]:
                raise ValueError(f"mask {m.shape} does not match image {a.shape[:2]}")
            if first is not None:
                s.update(yi1=torch.from_numpy(np.ascontiguousarray(first[2])), xi1=torch.from_numpy(np.ascontiguousarray(first[5])))
            s.update(mask=torch.from_numpy(m.copy()), yi=torch.from_numpy(np.ascontiguousarray(yi)),
                     xi=torch.from_numpy(np.ascontiguousarray(xi)))
        return s

    @staticmethod
    def randaug_fields(slots, width, height):
        """The slots ``RandAugment.draw`` returned -> (ra_op int32 [num_ops], ra_par float64 [num_ops, 8]) for ``mv_randaug_*``:
        code 0 = skipped, else index in RANDAUG_OPS + 1; geometric ops carry the 6 affine coefficients (Rotate's matrix built as
        ``Image.rotate`` builds it) + the filter (0 bilinear, 1 bicubic), the others their one argument."""
        from PIL import Image
        op, par = np.zeros(len(slots), np.int32), np.zeros((len(slots), 8), np.float64)
        for i, slot in enumerate(slots):
            if slot is None:
                continue
            name, arg, resample = slot
            op[i] = RANDAUG_OPS.index(name) + 1
            if name in RANDAUG_GEOMETRIC:
                par[i, :6] = affine_coefficients(name, arg, width, height)
                par[i, 6] = 1.0 if resample == Image.Resampling.BICUBIC else 0.0
            elif arg is not None:
                par[i, 0] = arg
        return op, par

    # ---- collate (worker) -------------------------------------------------------------------------------------
    @staticmethod
    def collate(batch):
        """batch: list of (sample dict, label | None).  Frames of different sizes are padded to the largest (the tables
        only address valid pixels); tap counts are padded to the batch maximum."""
        samples = [b[0] for b in batch]
        B = len(samples)
        Hs, Ws = max(s["raw"].shape[0] for s in samples), max(s["raw"].shape[1] for s in samples)
        ks = max(max(s["kh"].shape[1], s["kv"].shape[1]) for s in samples)
        if ks > MAX_TAPS:
            raise ValueError(f"downscale factor too large for the device path ({ks} taps)")
        oh, ow = samples[0]["kv"].shape[0], samples[0]["kh"].shape[0]
        labels = None if batch[0][1] is None else torch.as_tensor([b[1] for b in batch])
        has_mask = "mask" in samples[0]
        # frames (and masks): one stack when they share a shape -- the common case and the expensive copies (196 KB each)
        # --, zero-padded to the largest otherwise
        if all(s["raw"].shape == samples[0]["raw"].shape for s in samples):
            raw = torch.stack([s["raw"] for s in samples])
            mask = torch.stack([s["mask"] for s in samples]) if has_mask else None
        else:
            raw = torch.zeros(B, Hs, Ws, 3, dtype=torch.uint8)
            mask = torch.zeros(B, Hs, Ws, dtype=torch.uint8) if has_mask else None
            for i, s in enumerate(samples):
                h, w = s["raw"].shape[:2]
                raw[i, :h, :w] = s["raw"]
                if has_mask:
                    mask[i, :h, :w] = s["mask"]
        # tables: a few KB per sample; tap counts differ with the crop size (3 when upscaling, 5+ when downscaling)
        kh, kv = torch.zeros(B, ow, ks, dtype=torch.int32), torch.zeros(B, oh, ks, dtype=torch.int32)
        for i, s in enumerate(samples):
            if s["kv"].shape[0] != oh or s["kh"].shape[0] != ow:
                raise ValueError("samples of one batch must share the output size")
            kh[i, :, :s["kh"].shape[1]] = s["kh"]
            kv[i, :, :s["kv"].shape[1]] = s["kv"]
        out = {"raw": raw, "kh": kh, "bh": torch.stack([s["bh"] for s in samples]), "kv": kv,
               "bv": torch.stack([s["bv"] for s in samples]),
               "flip": torch.tensor([s["flip"] for s in samples], dtype=torch.uint8)}
        if has_mask:
            out.update(mask=mask, yi=torch.stack([s["yi"] for s in samples]), xi=torch.stack([s["xi"] for s in samples]))
        if "ra_op" in samples[0]:                                            # RandAugment: [B, num_ops] codes, [B, num_ops, 8] arguments
            out.update(ra_op=torch.stack([s["ra_op"] for s in samples]), ra_par=torch.stack([s["ra_par"] for s in samples]))
        if "kh1" in samples[0]:                                              # Resize -> RandomResizedCrop: stage-one tables
            k1 = max(max(s["kh1"].shape[1], s["kv1"].shape[1]) for s in samples)
            if k1 > MAX_TAPS:
                raise ValueError(f"downscale factor too large for the device path ({k1} taps)")
            S = samples[0]["kv1"].shape[0]
            kh1, kv1 = torch.zeros(B, S, k1, dtype=torch.int32), torch.zeros(B, S, k1, dtype=torch.int32)
            for i, s in enumerate(samples):
                kh1[i, :, :s["kh1"].shape[1]] = s["kh1"]
                kv1[i, :, :s["kv1"].shape[1]] = s["kv1"]
            out.update(kh1=kh1, kv1=kv1, bh1=torch.stack([s["bh1"] for s in samples]), bv1=torch.stack([s["bv1"] for s in samples]))
            if has_mask:
                out.update(yi1=torch.stack([s["yi1"] for s in samples]), xi1=torch.stack([s["xi1"] for s in samples]))
        return out, labels

    # ---- GPU side ---------------------------------------------------------------------------------------------
    def apply(self, packed, device, mask_add=0):
        """Packed CPU batch (pinned by the DataLoader) -> (images fp32 [B, 3, h, w], masks int64 [B, h, w] | None) on
        ``device``; the copies are asynchronous and the kernels run on the current stream."""
        from myrtle_vision.hip import ops
        d = {k: v.to(device, non_blocking=True) for k, v in packed.items()}
        raw, mask = d["raw"], d.get("mask")
        if "kh1" in d:                                                       # Resize first, as its own uint8 image
            raw = ops.image_resize_u8(raw, d["kh1"], d["bh1"], d["kv1"], d["bv1"])
            if mask is not None:
                mask = ops.mask_resize_u8(mask, d["yi1"], d["xi1"])
        if "ra_op" in d:
            return self._apply_randaug(ops, raw, d), None
        imgs = ops.image_prepare(raw, d["kh"], d["bh"], d["kv"], d["bv"], d["flip"], self.mean, self.std)
        masks = None
        if mask is not None:
            masks = ops.mask_prepare(mask, d["yi"], d["xi"], d["flip"], mask_add)
        return imgs, masks

    def _apply_randaug(self, ops, raw, d):
        """The chain with RandAugment: the last resampling kept as uint8 (``mv_image_resize_u8``), ``num_ops`` slots of two launches
        each, ping-ponging between two uint8 buffers, then ToTensor + Normalize by ``mv_image_prepare`` through copying tables."""
        img = ops.image_resize_u8(raw, d["kh"], d["bh"], d["kv"], d["bv"])
        B, oh, ow, _ = img.shape
        other, tables, mean = torch.empty_like(img), None, None
        for slot in range(d["ra_op"].shape[1]):
            tables, mean = ops.randaug_stats(img, d["ra_op"], slot, tables, mean)
            other = ops.randaug_apply(img, d["ra_op"], d["ra_par"], slot, tables, mean, self.randaug.fill, out=other)
            img, other = other, img
        key = (B, oh, ow, img.device)
        ident = self._identity.get(key)
        if ident is None:
            self._identity.clear()
            (bv, kv), (bh, kh) = (_identity_axis(np.arange(n)) for n in (oh, ow))
            dev = lambda a: torch.from_numpy(a).to(img.device).unsqueeze(0).expand(B, -1, -1).contiguous()
            ident = self._identity[key] = (dev(kh), dev(bh), dev(kv), dev(bv), torch.zeros(B, dtype=torch.uint8, device=img.device))
        return ops.image_prepare(img, *ident, self.mean, self.std)


# ---- detection: ragged batches ------------------------------------------------------------------------------------------
def _identity_axis(index):
    """Tables that copy: one tap of weight 1.0 on source pixel ``index[x]`` (the kernel's arithmetic returns the pixel itself)."""
    b = np.stack([index, np.ones_like(index)], axis=1).astype(np.int32)
    return b, np.full((len(index), 1), 1 << PRECISION_BITS, np.int32)


class TableFrame:
    """Stands in for the PIL image inside ``detection_transforms``' chain on the worker: it has the members that chain uses
    (``size`` / ``width`` / ``height``, ``crop``, ``transpose``, ``resize``) and, instead of touching pixels, records per axis
    how the current image is obtained from the last MATERIALISED uint8 image -- the decoded frame, or the result of an
    earlier resize, because Pillow rounds every resize to uint8 and a second one must start from that image.

    Before a resize the current image is a window of the materialised one, possibly mirrored: the index arrays ``gx`` / ``gy``.
    ``resize`` turns them into Pillow's resampling tables over that window (offsets folded into the bounds; a mirrored window
    reverses each row's taps, which leaves the integer sum unchanged).  After it, ``crop`` slices table rows and a flip
    reverses the row order.  A second ``resize`` closes the stage (``stages``) and starts over on its result."""

    def __init__(self, frame, tables=None):
        self.frame = frame                                     # uint8 [H, W, 3], the decoded image
        self.stages = []                                       # closed stages: (bv, kv, bh, kh)
        self.cur = None                                        # tables of the open stage, once it has resampled
        self.gy, self.gx = np.arange(frame.shape[0]), np.arange(frame.shape[1])
        self.norm = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
        self._tables = tables if tables is not None else bilinear_tables

    @property
    def height(self):
        return len(self.gy) if self.cur is None else len(self.cur[0])

    @property
    def width(self):
        return len(self.gx) if self.cur is None else len(self.cur[2])

    @property
    def size(self):
        return self.width, self.height

    def crop(self, box):
        left, top, right, bottom = box
        if not (0 <= left < right <= self.width and 0 <= top < bottom <= self.height):
            raise ValueError(f"crop box {box} outside the {self.size} image")
        if self.cur is None:
            self.gy, self.gx = self.gy[top:bottom], self.gx[left:right]
        else:
            bv, kv, bh, kh = self.cur
            self.cur = (bv[top:bottom], kv[top:bottom], bh[left:right], kh[left:right])
        return self

    def transpose(self, method):
        from PIL import Image
        if method != Image.Transpose.FLIP_LEFT_RIGHT:
            raise ValueError("only FLIP_LEFT_RIGHT is supported on the device path")
        if self.cur is None:
            self.gx = self.gx[::-1]
        else:
            bv, kv, bh, kh = self.cur
            self.cur = (bv, kv, bh[::-1], kh[::-1])
        return self

    def resize(self, size, resample=None):
        ow, oh = size
        w, h = self.size
        if (ow, oh) == (w, h):
            return self                                        # Pillow returns a copy
        if self.cur is not None:
            self.stages.append(self.cur)
            self.cur, self.gy, self.gx = None, np.arange(h), np.arange(w)
        bv, kv = self._tables(h, oh)
        bh, kh = self._tables(w, ow)
        bv, bh = bv.copy(), bh.copy()
        first, last = self.gx[bh[:, 0]], self.gx[bh[:, 0] + bh[:, 1] - 1]
        if len(self.gx) > 1 and self.gx[0] > self.gx[-1]:      # mirrored window: taps run right to left in the source
            j = bh[:, 1:2] - 1 - np.arange(kh.shape[1])[None, :]
            kh = np.where(j >= 0, np.take_along_axis(kh, np.maximum(j, 0), axis=1), 0).astype(np.int32)
            first = last
        bh[:, 0] = first
        bv[:, 0] = self.gy[bv[:, 0]]
        self.cur = (bv, kv, bh, kh)
        return self

    def normalized(self, mean, std):
        self.norm = (tuple(float(v) for v in mean), tuple(float(v) for v in std))
        return self

    def finish(self):
        """-> the sample dict: the frame, the final stage's tables and, if there was one, the first stage's."""
        if self.cur is None:
            bv, kv = _identity_axis(self.gy)
            bh, kh = _identity_axis(self.gx)
            self.cur = (bv, kv, bh, kh)
        if len(self.stages) > 1:
            raise ValueError("more than two resamplings in one chain are not supported on the device path")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
        s = {"raw": torch.from_numpy(np.ascontiguousarray(self.frame))}
        s.update(zip(("bv", "kv", "bh", "kh"), map(t, self.cur)))
        if self.stages:
            s.update(zip(("bv1", "kv1", "bh1", "kh1"), map(t, self.stages[0])))
        return s


def _pack_stage(samples, names, src_hw):
    """Per-sample tables of one stage -> padded [B, Hmax, ks] / [B, Wmax, ks] arrays + extents.  ``src_hw[i]`` is the size of
    the image sample i's tables address: every bound is checked against it here, on the host, before anything is launched."""
    bvn, kvn, bhn, khn = names
    B = len(samples)
    oh, ow = max(s[kvn].shape[0] for s in samples), max(s[khn].shape[0] for s in samples)
    ks = max(max(s[khn].shape[1], s[kvn].shape[1]) for s in samples)
    if ks > MAX_TAPS:
        raise ValueError(f"downscale factor too large for the device path ({ks} taps)")
    kh, kv = torch.zeros(B, ow, ks, dtype=torch.int32), torch.zeros(B, oh, ks, dtype=torch.int32)
    bh, bv = torch.zeros(B, ow, 2, dtype=torch.int32), torch.zeros(B, oh, 2, dtype=torch.int32)
    ext = torch.zeros(B, 2, dtype=torch.int32)
    for i, s in enumerate(samples):
        h, w = s[kvn].shape[0], s[khn].shape[0]
        for b, n in ((s[bvn], src_hw[i][0]), (s[bhn], src_hw[i][1])):
            if int(b[:, 0].min()) < 0 or int((b[:, 0] + b[:, 1]).max()) > n or int(b[:, 1].min()) < 1:
                raise ValueError("resampling table addresses pixels outside its source image")
        kh[i, :w, :s[khn].shape[1]], kv[i, :h, :s[kvn].shape[1]] = s[khn], s[kvn]
        bh[i, :w], bv[i, :h] = s[bhn], s[bvn]
        ext[i, 0], ext[i, 1] = h, w
    return {"kh": kh, "bh": bh, "kv": kv, "bv": bv, "ext": ext}


class DetectionDevicePlan:
    """Built from a detection ``transform_ops_*`` section.  ``plan(pil_image, target)`` (worker) runs the host chain of
    ``detection_transforms.from_config`` on a ``TableFrame``: the same draws, the same box / label / area arithmetic by the
    same functions, and tables instead of pixels.  ``collate`` pads frames and tables; ``apply`` runs the ragged kernels and
    returns the ``NestedTensor`` the host ``collate_fn`` would have built."""

    def __init__(self, transform_config=None, chain=None):
        from myrtle_vision.datasets.detection_transforms import from_config
        self.chain = chain if chain is not None else from_config(transform_config)     # ``chain``: an already built Compose
        self._cache = {}

    def _tables(self, n_in, n_out):
        t = self._cache.get((n_in, n_out))
        if t is None:
            if len(self._cache) > 4096:
                self._cache.clear()
            t = self._cache[(n_in, n_out)] = bilinear_tables(n_in, n_out)
        return t

    def __call__(self, img, target):
        frame = TableFrame(np.asarray(img.convert("RGB"), dtype=np.uint8).copy(), self._tables)
        out, target = self.chain(frame, target)
        if out is not frame:
            raise ValueError("transform chain not supported on the device path")
        sample = frame.finish()
        sample["mean"], sample["std"] = frame.norm
        return sample, target

    @staticmethod
    def collate(batch):
        """[(sample dict, target), ...] -> (packed dict of CPU tensors, tuple of targets).  A batch may mix one- and
        two-resampling samples (RandomSelect draws per image): a one-resampling sample then gets a copying first stage."""
        samples, targets = [b[0] for b in batch], tuple(b[1] for b in batch)
        B = len(samples)
        raw_hw = [tuple(s["raw"].shape[:2]) for s in samples]
        Hs, Ws = max(h for h, _ in raw_hw), max(w for _, w in raw_hw)
        raw = torch.zeros(B, Hs, Ws, 3, dtype=torch.uint8)
        for i, s in enumerate(samples):
            raw[i, :raw_hw[i][0], :raw_hw[i][1]] = s["raw"]
        norms = {(tuple(map(float, s["mean"])), tuple(map(float, s["std"]))) for s in samples}
        if len(norms) != 1:                                    # the kernel takes ONE mean / std per launch
            raise ValueError("samples of one batch must share the normalisation")
        out = {"raw": raw, "norm": torch.tensor(list(norms.pop()), dtype=torch.float64)}
        src_hw = raw_hw
        if any("kh1" in s for s in samples):
            staged = []
            for s, (h, w) in zip(samples, raw_hw):
                if "kh1" not in s:
                    s = dict(s)
                    (s["bv1"], s["kv1"]), (s["bh1"], s["kh1"]) = (tuple(map(torch.from_numpy, _identity_axis(np.arange(n))))
                                                                    for n in (h, w))
                staged.append(s)
            samples = staged
            first = _pack_stage(samples, ("bv1", "kv1", "bh1", "kh1"), raw_hw)
            out.update({k + "1": v for k, v in first.items()})
            src_hw = [tuple(int(v) for v in e) for e in first["ext"]]
        out.update(_pack_stage(samples, ("bv", "kv", "bh", "kh"), src_hw))
        return out, targets

    @staticmethod
    def output_shapes(packed):
        """-> (images, mask, intermediate | None) shapes of ``apply`` for a packed batch."""
        B, oh, ow = packed["kv"].shape[0], packed["kv"].shape[1], packed["kh"].shape[1]
        first = (B, packed["kv1"].shape[1], packed["kh1"].shape[1], 3) if "kh1" in packed else None
        return (B, 3, oh, ow), (B, oh, ow), first

    def apply(self, packed, device, out=None, mask=None, stage_out=None):
        """Packed CPU batch -> ``NestedTensor`` (images fp32 [B, 3, Hmax, Wmax], padding mask bool [B, Hmax, Wmax]) on ``device``.
        ``out`` / ``mask`` / ``stage_out``: preallocated results and uint8 intermediate (see ``output_shapes``)."""
        from myrtle_vision.datasets.detection_transforms import NestedTensor
        from myrtle_vision.hip import ops
        mean, std = (tuple(float(v) for v in row) for row in packed["norm"])
        d = {k: v.to(device, non_blocking=True) for k, v in packed.items() if k != "norm"}
        raw = d["raw"]
        if "kh1" in d:
            raw = ops.image_resize_u8_ragged(raw, d["kh1"], d["bh1"], d["kv1"], d["bv1"], d["ext1"], out=stage_out)
        imgs, mask = ops.image_prepare_ragged(raw, d["kh"], d["bh"], d["kv"], d["bv"], d["ext"], mean, std, out=out, mask=mask)
        return NestedTensor(imgs, mask)
