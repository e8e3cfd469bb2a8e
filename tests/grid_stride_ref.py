"""What tests/test_grid_stride_gpu.py shares between its tests: guarded device buffers, the library handle, and the CPU restatements
that are longer than a line.  Not a test module."""
import math

import numpy as np
import torch

MV_OK = 0
MV_F32, MV_BF16, MV_I8, MV_F16 = 0, 1, 2, 3
DT = {torch.float32: MV_F32, torch.bfloat16: MV_BF16, torch.int8: MV_I8, torch.float16: MV_F16}


def L():
    from myrtle_vision.hip.lib import lib
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


def relerr(got, want):
    """max|got - want| / max|want|: the measure of tests/test_hip_ops.py."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


class Arena:
    """Every tensor is a 16-byte-aligned view in the middle of its own allocation with GUARD canary bytes on both sides.  Outputs
    are pre-filled: NaN for floating types, the byte 0x7f for integer types, so an element no kernel wrote is visible.  ``check()``
    synchronises and asserts that both canaries of every buffer are intact and that no element of an output made since the last
    check still holds its pre-fill."""
    GUARD, CANARY, PREFILL = 4096, 0xA5, 0x7F

    def __init__(self):
        self.raws, self.fresh = [], []

    def _carve(self, shape, dtype):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        nbytes = math.prod(shape) * torch.empty((), dtype=dtype).element_size()
        raw = torch.full((nbytes + 2 * self.GUARD,), self.CANARY, dtype=torch.uint8, device="cuda")
        body = raw[self.GUARD:self.GUARD + nbytes].view(dtype).view(shape)
        assert body.data_ptr() % 16 == 0
        self.raws.append(raw)
        return body

    def inp(self, data, dtype=None):
        """A guarded copy of ``data`` (a CPU or device tensor): inputs, and outputs that a call accumulates into."""
        body = self._carve(data.shape, dtype or data.dtype)
        body.copy_(data)
        return body

    def out(self, shape, dtype):
        body = self._carve(shape, dtype)
        if body.is_floating_point():
            body.fill_(float("nan"))
        else:
            body.view(torch.uint8).fill_(self.PREFILL)
        self.fresh.append(body)
        return body

    def scratch(self, nbytes):
        """A guarded workspace: a kernel may leave parts of it unwritten."""
        return self._carve((max(int(nbytes), 16),), torch.uint8)

    @classmethod
    def prefill_of(cls, dtype):
        return int.from_bytes(bytes([cls.PREFILL]) * torch.empty((), dtype=dtype).element_size(), "little")

    def check(self):
        try:
            torch.cuda.synchronize()
        except RuntimeError as e:                       # a device fault: nothing more may start on this device in this session
            import pytest
            pytest.exit(f"the device reported a fault, stopping the session: {e}", returncode=3)
        g = self.GUARD
        for raw in self.raws:
            assert bool((raw[:g] == self.CANARY).all()) and bool((raw[-g:] == self.CANARY).all()), "a kernel wrote outside its tensor"
        for body in self.fresh:
            if body.is_floating_point():
                left = int(torch.isnan(body).sum())
            else:
                left = int((body == self.prefill_of(body.dtype)).sum())
            assert left == 0, f"{left} of {body.numel()} output elements were never written"
        self.fresh = []

    def free(self):
        self.raws, self.fresh = [], []
        torch.cuda.empty_cache()


def tiled(base, n):
    """``base`` (1-D) repeated to n elements: inputs and references of position-independent operations."""
    return base.repeat((n + base.numel() - 1) // base.numel())[:n]


def small_ints(shape, seed, dtype=torch.float32):
    """Uniform integers -8 .. 8: exact in bf16 and fp32, so a sum of fewer than 2^24 / 8 of them is exact in any order."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, tuple(shape), generator=g, dtype=torch.int8).to(dtype)


def split_pieces(x):
    """The three bf16 pieces of an fp32 tensor (csrc/elementwise.hip, split3_kernel): p0 = bf16(x), p1 = bf16(x - p0),
    p2 = bf16(x - p0 - p1), each subtraction exact in fp32."""
    p0 = x.to(torch.bfloat16)
    r1 = x - p0.float()
    p1 = r1.to(torch.bfloat16)
    p2 = (r1 - p1.float()).to(torch.bfloat16)
    return p0, p1, p2


SPLIT_ORDER = {0: (0, 0, 1, 0, 1, 2), 1: (0, 1, 0, 2, 1, 0)}        # which piece each of the six segments holds, per role


def dgelu64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * np.pi) ** 0.5


def affine_codes_ref(x, scale, zp):
    """The integer codes q - zp of the quint8 quantiser, as tests/test_hip_ops.py::test_int8_codes_gemm_equals_fake_quant_linear
    restates them: round(fake_quantize(x) / scale)."""
    xq = torch.fake_quantize_per_tensor_affine(x.float(), scale, zp, 0, 255)
    return torch.round(xq / scale)


def grad_norm_ref(g, grad_scale, max_norm):
    """(exact sum of squares, total, coefficient of a total): total = float32(sqrt(S)) * float32(grad_scale);
    coefficient(t) = min(1, float32(max_norm) / (t + float32(1e-6))), all in fp32 as csrc/elementwise.hip writes it."""
    f32 = np.float32
    S = int((g.to(torch.int64) ** 2).sum())
    total = f32(f32(math.sqrt(S)) * f32(grad_scale))

    def coef(t):
        c = f32(f32(max_norm) / f32(f32(t) + f32(1e-6)))
        return c if c < f32(1.0) else f32(1.0)
    return S, total, coef
