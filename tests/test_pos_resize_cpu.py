"""Positional-embedding resize without a GPU: the library exports the two entry points and lib.py declares them, the caps of ops.py
agree with the argument checks of the library, and the tap / weight formulas the kernels are written to (include/myrtle_vision_hip.h,
mv_pos_resize_fwd) reproduce torch's CPU ``F.interpolate(mode="bicubic", align_corners=False)``."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                      # 16-byte aligned, never dereferenced: the probes below stop at an argument check
ENTRIES = ("mv_pos_resize_fwd", "mv_pos_resize_bwd")


def test_library_exports_the_entry_points_and_lib_declares_them():
    from myrtle_vision.hip import lib
    from myrtle_vision.hip.build import LIB_PATH
    assert lib.SIGNATURES["mv_pos_resize_fwd"] == ("pp" "iiiii" "p", ctypes.c_int)
    assert lib.SIGNATURES["mv_pos_resize_bwd"] == ("ppi" "iiiii" "p", ctypes.c_int)
    raw = ctypes.CDLL(LIB_PATH)                                   # the built library itself, not the declarations
    for name in ENTRIES:
        assert getattr(raw, name) is not None
    handle = lib.lib()
    assert handle.mv_pos_resize_fwd.argtypes[2:7] == [ctypes.c_int] * 5


def probe(entry, sh, sw, gh, gw, D, addr=ADDR + 4):
    """Call ``entry`` with a MISALIGNED dummy address: dimension checks come first, so arguments the library takes end in
    MV_ERR_ALIGN and arguments it refuses in their own code; nothing is launched either way (no device needed)."""
    from myrtle_vision.hip import lib
    fn = getattr(lib.lib(), entry)
    if entry.endswith("fwd"):
        return fn(addr, addr, sh, sw, gh, gw, D, None)
    return fn(addr, addr, 0, sh, sw, gh, gw, D, None)


@pytest.mark.parametrize("entry", ENTRIES)
def test_supported_agrees_with_the_library_at_each_limit(entry):
    from myrtle_vision.hip import ops
    cap = ops.POS_RESIZE_MAX_SIDE
    assert cap == 1024 and cap >= 512                             # the header's stated cap; the least the model needs is 512
    # (sh, sw, gh, gw, D) -> the code of the first check that refuses it
    cases = [((14, 14, cap, cap, 4), ALIGN), ((14, 14, cap + 1, 20, 4), UNSUPPORTED), ((14, 14, 20, cap + 1, 4), UNSUPPORTED),
             ((cap, cap, 3, 5, 64), ALIGN), ((cap + 1, 14, 3, 5, 64), UNSUPPORTED), ((14, cap + 1, 3, 5, 64), UNSUPPORTED),
             ((14, 14, 1, 1, 4), ALIGN), ((14, 14, 0, 1, 4), SHAPE), ((14, 14, 1, 0, 4), SHAPE), ((0, 14, 1, 1, 4), SHAPE),
             ((14, 14, 20, 33, 768), ALIGN), ((14, 14, 20, 33, 6), SHAPE), ((14, 14, 20, 33, 2), SHAPE), ((14, 14, 20, 33, 0), SHAPE)]
    for (sh, sw, gh, gw, D), code in cases:
        assert probe(entry, sh, sw, gh, gw, D) == code, (sh, sw, gh, gw, D)
        assert ops.pos_resize_supported(D, gh, gw, sh, sw) == (code == ALIGN), (sh, sw, gh, gw, D)
    assert probe(entry, 14, 14, 3, 5, 64, addr=0) == ALIGN        # NULL is refused too
    assert ops.pos_resize_supported(64, 3, 5) and not ops.pos_resize_supported(6, 3, 5)          # the model's 14 x 14 default


# ---------------------------------------------------------------------------------------------- the specification
def taps(n_out, n_in):
    """Per axis, in fp32 as the kernels compute it: src = (dst + 0.5) * (in / out) - 0.5 (not clamped), i = floor(src), t = src - i,
    taps i-1 .. i+2 with indices clamped to [0, in-1], cubic-convolution weights with A = -0.75.  -> (idx [n_out, 4], w [n_out, 4])."""
    f = np.float32
    A = f(-0.75)
    scale = f(n_in) / f(n_out)
    dst = np.arange(n_out, dtype=f)
    src = scale * (dst + f(0.5)) - f(0.5)
    i = np.floor(src)
    t = (src - i).astype(f)

    def inner(x):
        return ((A + f(2)) * x - (A + f(3))) * x * x + f(1)

    def outer(x):
        return ((A * x - f(5) * A) * x + f(8) * A) * x - f(4) * A

    w = np.stack([outer(t + f(1)), inner(t), inner(f(1) - t), outer((f(1) - t) + f(1))], axis=1).astype(f)
    idx = np.clip(i.astype(np.int64)[:, None] + np.arange(-1, 3)[None, :], 0, n_in - 1)
    return idx, w


def weight_matrix(sh, sw, gh, gw):
    """R [gh*gw, sh*sw] of the restated formulas (fp64 products of the fp32 per-axis weights; clamped taps add up on their cell)."""
    iy, wy = taps(gh, sh)
    ix, wx = taps(gw, sw)
    R = np.zeros((gh * gw, sh * sw))
    for y in range(gh):
        for x in range(gw):
            for j in range(4):
                for i in range(4):
                    R[y * gw + x, iy[y, j] * sw + ix[x, i]] += float(wy[y, j]) * float(wx[x, i])
    return R


@pytest.mark.parametrize("grid", [(3, 5), (16, 16), (20, 33), (1, 1)])
def test_the_tap_formulas_reproduce_torch_bicubic(grid):
    gh, gw = grid
    sh = sw = 14
    eye = torch.eye(sh * sw, dtype=torch.float32).reshape(1, sh * sw, sh, sw)           # channel q = the one-hot grid of cell q
    want = TF.interpolate(eye, size=grid, mode="bicubic", align_corners=False).reshape(sh * sw, gh * gw).t().numpy()
    got = weight_matrix(sh, sw, gh, gw)
    # Two fp32 evaluations of the same formulas (torch's build may contract a * b + c into one fma, this restatement rounds every
    # operation): src < 16 may differ by one ulp = 2^-20, times |dw/dt| < 1.2; the Horner steps of the outer weight pass through
    # values up to 8|A| = 6 that cancel, about 30 * 2^-24 in all; together under 3e-6 per axis, and the 2-D weight is a product
    # with a second weight of size at most 1.2 on either side: 2^-17 = 7.6e-6.  A shifted, swapped or unclamped tap is off by 1e-2.
    err = np.abs(got - want).max()
    print(f"grid {grid}: max |restated - torch fp32| = {err:.3e}")
    assert err <= 2.0 ** -17
    assert np.abs(got.sum(axis=1) - 1.0).max() <= 2.0 ** -17                            # a constant resizes to itself, to the same roundings
    if grid == (3, 5):
        assert (np.abs(got).sum(axis=0) == 0).any()                                     # downscaling: four taps, no antialiasing
    idx, w = taps(14, 14)
    assert np.array_equal(w, np.tile(np.float32([0, 1, 0, 0]), (14, 1))) and np.array_equal(idx[:, 1], np.arange(14))
