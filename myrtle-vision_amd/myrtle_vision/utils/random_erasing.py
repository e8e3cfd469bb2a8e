"""Random Erasing of a device batch, in place, on the HIP kernels (``mv_random_erase_draw`` / ``mv_random_erase_apply``).

A restatement of timm's ``timm.data.random_erasing.RandomErasing`` (Zhong et al., "Random Erasing Data Augmentation", 2017; DeiT's
``--reprob 0.25 --remode pixel --recount 1``): per sample, with ``probability``, ``count`` boxes of a log-uniform aspect ratio and a
uniform share of the image's area, up to ten attempts each, filled with zeros (``const``), one normal value per channel (``rand``) or
one per element (``pixel``).  timm is not available offline and the reference never erases, so the SOURCE of the random draws is
a restatement too (PARITY UNPINNED against timm, as ``utils/mixup.py`` says of its own): timm draws from Python's ``random`` and
torch's generator on the host, one sample at a time; this class draws every box in ONE launch from the project's Philox stream
(``csrc/random_erase.hip`` fixes the counter of every word) and fills them in a second one.  ``tests/random_erase_ref.py`` pins
that definition bit for bit.
"""
import math

import torch

MODES = ("const", "rand", "pixel")


class RandomErasing:
    """``eraser(imgs) -> imgs``: erases the [B, Ch, H, W] device batch IN PLACE.  A plain object, not a module -- no parameter, no
    buffer, no state-dict key.  The arguments carry timm's defaults and its meaning of ``None``: ``max_aspect=None`` is
    ``1 / min_aspect``, ``max_count=None`` is ``min_count``.

    The device array ``state`` int64 [2] = (seed, step) is created by the first call.  The draw reads it on the device and leaves
    step + 1 behind: no host read and no host scalar that changes, so -- unlike ``Mixup`` -- a captured training step
    (``utils/graph.py``) may contain an eraser and erases anew on every replay.  The initial seed comes from torch's CPU generator
    at the first call (``seed_everything`` reproduces it; ``seed(int)`` sets it); the process's distributed rank is added, because
    every rank is seeded alike and ranks must not share boxes.  NOT checkpointed: a resumed run draws a new seed."""

    def __init__(self, probability=0.25, mode="pixel", min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
                 max_count=None):
        from myrtle_vision.hip.ops import RANDOM_ERASE_MAX_COUNT
        if not 0.0 < min_aspect < math.inf:
            raise ValueError(f"0 < min_aspect expected, got {min_aspect}")
        max_aspect = 1.0 / min_aspect if max_aspect is None else max_aspect
        max_count = min_count if max_count is None else max_count
        if not 0.0 <= probability <= 1.0:                         # a NaN fails every one of these
            raise ValueError(f"probability has to be in [0, 1], got {probability}")
        if mode not in MODES:
            raise ValueError(f"mode is one of {MODES}, got {mode!r}")
        if not 0.0 < min_area <= max_area <= 1.0:
            raise ValueError(f"0 < min_area <= max_area <= 1 expected, got {min_area} and {max_area}")
        if not 0.0 < max_aspect < math.inf:
            raise ValueError(f"a finite max_aspect > 0 expected, got {max_aspect}")
        if int(min_count) != min_count or int(max_count) != max_count or not 1 <= min_count <= max_count <= RANDOM_ERASE_MAX_COUNT:
            raise ValueError(f"1 <= min_count <= max_count <= {RANDOM_ERASE_MAX_COUNT} expected, got {min_count} and {max_count}")
        self.probability, self.mode = float(probability), mode
        self.min_area, self.max_area = float(min_area), float(max_area)
        lo, hi = math.log(min_aspect), math.log(max_aspect)
        self.log_ratio = (min(lo, hi), max(lo, hi))               # timm's random.uniform takes the two in either order
        self.min_count, self.max_count = int(min_count), int(max_count)
        self.thr = int(self.probability * 4294967296.0)           # 2**32 at probability 1: every 32-bit word is below it
        self._seed = None                # drawn at the first call: building an eraser leaves the generator alone
        self._step = 0
        self._dev = None                 # (device, state)
        self.last_boxes = None           # int32 [B, max_count, 4] of the last call

    def seed(self, seed: int, step: int = 0):
        """Restart the stream at (seed + rank, step)."""
        self._seed, self._step, self._dev = int(seed), int(step), None

    @staticmethod
    def _rank():
        dist = torch.distributed
        return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def _state(self, device):
        device = torch.device(device)
        if self._dev is None or self._dev[0] != device:
            if self._dev is not None:                             # the batches moved: carry the stream over
                self._seed, self._step = (int(v) for v in self._dev[1].tolist())
                self._seed -= self._rank()
            if self._seed is None:
                self._seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64))
            self._dev = (device, torch.tensor([self._seed + self._rank(), self._step], dtype=torch.int64).to(device))
        return self._dev[1]

    @property
    def state(self):
        """Device int64 [2] = (seed, step), or None before the first call."""
        return None if self._dev is None else self._dev[1]

    def __call__(self, imgs):
        if self.probability == 0.0:
            return imgs                          # nothing is drawn, nothing is launched
        from myrtle_vision.hip import ops
        if not imgs.is_contiguous():
            imgs = imgs.contiguous()             # the kernel walks a dense batch; the caller goes on with the returned tensor
        B, _, H, W = imgs.shape
        boxes, used = ops.random_erase_draw(self._state(imgs.device), B, H, W, thr=self.thr, min_area=self.min_area,
                                            max_area=self.max_area, log_ratio=self.log_ratio, min_count=self.min_count,
                                            max_count=self.max_count)
        self.last_boxes = boxes
        return ops.random_erase_apply(imgs, boxes, used, self.mode)
