"""Reference restatements for the drop-path tests (TEST INFRASTRUCTURE, imported by test_drop_path_cpu.py / _gpu.py).

The draw: ``mv_drop_path_draw`` is ``mv_dropout``'s Philox mask over R * B elements with offset = step, so row r of the table is
``oracle.dropout_oracle.dropout_keep_mask(R * B, p_r, seed, step)[r * B:(r + 1) * B]`` times float32(1 / (1 - p_r)).
The block: the parent behaviour composed with torch ops, x + c[:, None, None] * (block(x) - x).
"""
import numpy as np

from oracle.dropout_oracle import dropout_keep_mask


def keep_rows(rates, B, seed, step):
    """bool [R, B]: which (branch, sample) pairs survive."""
    R = len(rates)
    return np.stack([dropout_keep_mask(R * B, p, seed, step)[r * B:(r + 1) * B] for r, p in enumerate(rates)]) if R else \
        np.zeros((0, B), dtype=bool)


def draw_table(rates, B, seed, step):
    """float32 [R, B]: the table ``mv_drop_path_draw`` writes for (seed, step)."""
    keep = keep_rows(rates, B, seed, step)
    scale = np.array([np.float32(1.0 / (1.0 - p)) for p in rates], dtype=np.float32).reshape(-1, 1)
    return np.where(keep, scale, np.float32(0.0)).astype(np.float32)


def composed(block, x, c):
    """x + c * (block(x) - x) with torch ops on x's device: ``block`` is the parent's residual branch, x + f(LN(x))."""
    return x + c.view(-1, *([1] * (x.dim() - 1))) * (block(x) - x)


class Guarded:
    """Tensors allocated between sentinel zones: ``new(shape, dtype)`` gives a view whose neighbours hold a known pattern,
    ``check()`` asserts that no kernel wrote outside.  GUARD elements of the tensor's own dtype on each side (a multiple of 16
    bytes, so the view keeps the 16-byte alignment the kernels ask for)."""
    GUARD = 64

    def __init__(self, torch, device="cuda"):
        self.torch, self.device, self.zones = torch, device, []

    def new(self, shape, dtype, fill=None):
        torch = self.torch
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * self.GUARD,), -77.0, dtype=dtype, device=self.device)
        view = buf[self.GUARD:self.GUARD + n].view(*shape)
        if fill is not None:
            view.copy_(fill)
        else:
            view.fill_(float("nan"))
        self.zones.append(buf)
        return view

    def check(self):
        torch = self.torch
        for buf in self.zones:
            g = self.GUARD
            assert bool((buf[:g] == -77.0).all()) and bool((buf[-g:] == -77.0).all()), "a kernel wrote outside its tensor"
