"""Reference restatements for the Random Erasing tests (TEST INFRASTRUCTURE, imported by test_random_erase_cpu.py / _gpu.py).

Written from the header comment of ``csrc/random_erase.hip``, over ``oracle.dropout_oracle.philox4x32_10``: every word is
Philox4x32-10(counter = (index lo, (tag << 24) | index hi, step lo, step hi), key = seed) with

* tag 1, the box draw: index = b * 128 + j; j = 0 holds the sample word (0) and the count word (1), j = 1 + k * 10 + a the four
  words (area, aspect, top, left) of attempt a of erase k;
* tag 2, the colours of mode ``rand``: index = (b * 8 + k) * Ch + channel, words (0, 1), the cos branch;
* tag 3, the noise of mode ``pixel``: index = i >> 2 for flat element i, words (i & 2, (i & 2) + 1), cos for even i, sin for odd i.

The draw is fp64 throughout, as in the kernel (python floats are IEEE doubles; ``round`` rounds half to even): only ``exp`` and
``sqrt`` can differ from the device's, by an ulp, which matters only where the value under ``round`` sits on a half-integer --
``draw`` returns those values so a test can tell.  The fill is Box-Muller in fp64 on the uniforms ((word >> 9) + 0.5) * 2^-23, which
are exact in fp32: the kernel's fp32 evaluation differs from it by rounding alone.
"""
import math

import numpy as np

from drop_path_ref import Guarded  # noqa: F401  (the guard zones of the GPU tests)
from oracle.dropout_oracle import philox4x32_10

TAG_DRAW, TAG_COLOUR, TAG_PIXEL = 1, 2, 3
ATTEMPTS, MAX_COUNT, SAMPLE_STRIDE = 10, 8, 128
_M32 = np.uint64(0xFFFFFFFF)


def words(tag, index, seed, step):
    """uint64 [..., 4]: the four words of the Philox call ``index`` (array of python ints / uint64) of stream ``tag``."""
    index = np.asarray(index, dtype=np.uint64)
    step &= (1 << 64) - 1
    z = np.zeros(index.shape, dtype=np.uint64)
    c1 = np.uint64(tag << 24) | (index >> np.uint64(32))
    r = philox4x32_10(index & _M32, c1, z + np.uint64(step & 0xFFFFFFFF), z + np.uint64(step >> 32), seed & 0xFFFFFFFF,
                      (seed >> 32) & 0xFFFFFFFF)
    return np.stack(r, axis=-1)


def counters(tag, index, step):
    """The (c0, c1, c2, c3) tuples of those calls, as a set: what must never be shared between streams."""
    return {(int(i) & 0xFFFFFFFF, (tag << 24) | (int(i) >> 32), step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF) for i in np.ravel(index)}


def umulhi(word, n):
    return (int(word) * int(n)) >> 32


def draw(B, H, W, seed, step, probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, min_count=1,
         max_count=None):
    """-> (boxes int32 [B, max_count, 4] = (top, left, h, w), attempts, calls): what ``mv_random_erase_draw`` writes for (seed, step).
    ``attempts``: one (b, k, a, sqrt(target * ratio), sqrt(target / ratio)) per attempt made, the values BEFORE rounding.
    ``calls``: the tag-1 call indices the draw consumed."""
    max_aspect = 1.0 / min_aspect if max_aspect is None else max_aspect
    max_count = min_count if max_count is None else max_count
    thr = int(float(probability) * 4294967296.0)
    lo, hi = sorted((math.log(min_aspect), math.log(max_aspect)))
    area = float(H) * float(W)
    idx = np.arange(B, dtype=np.uint64)[:, None] * np.uint64(SAMPLE_STRIDE) + np.arange(1 + MAX_COUNT * ATTEMPTS, dtype=np.uint64)
    w = words(TAG_DRAW, idx, seed, step)                                   # [B, 81, 4]
    boxes = np.zeros((B, max_count, 4), dtype=np.int32)
    attempts, calls = [], []
    for b in range(B):
        calls.append(b * SAMPLE_STRIDE)
        if not int(w[b, 0, 0]) < thr:
            continue
        count = min_count + umulhi(w[b, 0, 1], max_count - min_count + 1)
        for k in range(count):
            for a in range(ATTEMPTS):
                j = 1 + k * ATTEMPTS + a
                calls.append(b * SAMPLE_STRIDE + j)
                ua, ur = (int(w[b, j, 0]) + 0.5) * 2.0 ** -32, (int(w[b, j, 1]) + 0.5) * 2.0 ** -32
                target = (min_area + ua * (max_area - min_area)) * area / float(count)
                ratio = math.exp(lo + ur * (hi - lo))
                sh, sw = math.sqrt(target * ratio), math.sqrt(target / ratio)
                attempts.append((b, k, a, sh, sw))
                h, ww = int(round(sh)), int(round(sw))
                if h < H and ww < W:
                    boxes[b, k] = (umulhi(w[b, j, 2], H - h + 1), umulhi(w[b, j, 3], W - ww + 1), h, ww)
                    break
    return boxes, attempts, calls


def near_half(attempts, eps=1e-6):
    """The attempts whose value under ``round`` lies within ``eps`` of a half-integer: where an ulp of exp / sqrt could turn it."""
    return [t for t in attempts if any(abs((v % 1.0) - 0.5) <= eps for v in t[3:])]


def normal64(a, b, sin_branch):
    """fp64 Box-Muller of the word pair (a, b) (uint64 arrays): sqrt(-2 ln u1) * cos(2 pi u2), or sin where ``sin_branch``."""
    u1 = ((np.asarray(a, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = ((np.asarray(b, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r, t = np.sqrt(-2.0 * np.log(u1)), 2.0 * np.pi * u2
    return r * np.where(sin_branch, np.sin(t), np.cos(t))


def pixel_words(i, seed, step):
    """(a, b, sin_branch) of flat element indices ``i``: the word pair and branch of mode ``pixel``."""
    i = np.asarray(i, dtype=np.uint64)
    w = words(TAG_PIXEL, i >> np.uint64(2), seed, step)
    second = (i & np.uint64(2)) != 0
    return np.where(second, w[..., 2], w[..., 0]), np.where(second, w[..., 3], w[..., 1]), (i & np.uint64(1)) != 0


def pixel_normals(i, seed, step):
    return normal64(*pixel_words(i, seed, step))


def colour_words(b, k, c, Ch, seed, step):
    w = words(TAG_COLOUR, (np.asarray(b, dtype=np.uint64) * np.uint64(MAX_COUNT) + np.uint64(k)) * np.uint64(Ch) + np.uint64(c), seed, step)
    return w[..., 0], w[..., 1], np.zeros(w.shape[:-1], dtype=bool)


def winners(boxes, H, W):
    """int [B, H, W]: the erase k that owns each pixel (boxes written in order: the LAST one wins), -1 outside every box."""
    boxes = np.asarray(boxes)
    out = np.full((boxes.shape[0], H, W), -1, dtype=np.int64)
    for b in range(boxes.shape[0]):
        for k in range(boxes.shape[1]):
            top, left, h, w = (int(v) for v in boxes[b, k])
            if h > 0 and w > 0:
                out[b, max(top, 0):min(top + h, H), max(left, 0):min(left + w, W)] = k
    return out


def fill64(shape, boxes, mode, seed, step):
    """-> (owner int [B, H, W], values fp64 [B, Ch, H, W]): the fill of ``mv_random_erase_apply`` in fp64; ``values`` is meaningful
    where owner >= 0."""
    B, Ch, H, W = shape
    owner = winners(boxes, H, W)
    values = np.zeros(shape, dtype=np.float64)
    if mode == "pixel":
        values = pixel_normals(np.arange(B * Ch * H * W, dtype=np.uint64), seed, step).reshape(shape)
    elif mode == "rand":
        for b in range(B):
            for k in range(np.asarray(boxes).shape[1]):
                for c in range(Ch):
                    values[b, c][owner[b] == k] = float(normal64(*colour_words(b, k, c, Ch, seed, step)))
    return owner, values


def bf16_round(x32):
    """float32 array -> the bf16 value nearest to each element (ties to even), as float32."""
    bits = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = ((bits + np.uint64(0x7FFF) + ((bits >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return bits.astype(np.uint32).view(np.float32)
