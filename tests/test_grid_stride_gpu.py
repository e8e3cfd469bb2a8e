"""The grid-stride kernels of the older half of the hot path, past their launch caps.

csrc/elementwise.hip (ew_grid), the softmax pair of csrc/gemm_f32.hip, LayerNorm forward, the soft-target and distillation losses
launch at most a fixed number of workgroups and walk the rest of their input in a loop.  Every size here is one pass of the capped
grid plus five workgroups' worth plus a ragged tail (tests/test_grid_caps_cpu.py holds the caps and pins them to the sources), so
some threads run two iterations, some one, and the scalar tail loops run.  Two smaller gaps ride along: every width class of
ln_fwd_kernel, and mv_colsum called directly on each of its paths.

Conventions: the C entry points are called through ``lib()`` on guarded buffers (grid_stride_ref.Arena: canaries on both sides,
outputs pre-filled with NaN or 0x7f; ``A.check()`` after every call).  Comparisons are bit for bit wherever the operation is
reproducible, over the whole output; otherwise the bar is the one tests/test_hip_ops.py applies to the same entry point, quoted at
the check.  Reductions run on integers -8 .. 8, for which every summation order gives the same bits and the reference is an int64
sum.  Two bars are measured, not quoted (softmax backward; LayerNorm mean / rstd): 8 x the error of a plain fp32 torch evaluation
on the CPU against fp64 on the same inputs -- two reduction orders and one reassociation of headroom."""
import numpy as np
import pytest
import torch

import distill_ref
from grid_stride_ref import (DT, MV_BF16, MV_F32, MV_OK, SPLIT_ORDER, Arena, L, affine_codes_ref, dgelu64, grad_norm_ref, ptr,
                             relerr, small_ints, split_pieces, stream, tiled)
from mixup_ref import soft_target
from oracle import quant_oracle
from oracle.dropout_oracle import dropout_keep_mask
from oracle.vit_oracle import gelu_erf, layer_norm as ln_oracle, patchify as patchify_oracle
from test_grid_caps_cpu import N_S1, N_SUMSQ, N_V4, R_LN, R_W4, one_pass

pytestmark = pytest.mark.gpu

F32, BF16, F16, I8, I64 = torch.float32, torch.bfloat16, torch.float16, torch.int8, torch.int64
PERIOD = 65_521                          # a prime: the tiled inputs of the elementwise tests never line up with a workgroup or a pass
Q_SCALE, Q_ZERO = 0.05, 100              # quint8 quantiser of the code tests: inputs in [-6, 6] clamp at level 0 and stay below 255


def g(seed):
    return torch.Generator().manual_seed(seed)


@pytest.fixture
def A():
    arena = Arena()
    yield arena
    arena.free()


def ok(rc):
    assert rc == MV_OK, rc


def bits_equal(got, want):
    """Same dtype, same shape, same bits (so -0.0 and NaN payloads count)."""
    got, want = got.cpu().contiguous(), want.cpu().contiguous()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    view = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[got.element_size()]
    return torch.equal(got.view(view), want.view(view))


# ================================================================== 1. exact elementwise, 16 bytes per thread
def test_cast_every_built_pair(A):
    assert N_V4 > one_pass("ew_v4")
    base = torch.randn(PERIOD, generator=g(1))
    x = tiled(base, N_V4)
    for src, dst in [(F32, BF16), (BF16, F32), (F32, F32), (F32, F16)]:
        xs = x.to(src)
        xd, yd = A.inp(xs), A.out((N_V4,), dst)
        ok(L().mv_cast(ptr(xd), DT[src], ptr(yd), DT[dst], N_V4, stream()))
        A.check()
        assert bits_equal(yd, xs.to(dst)), (src, dst)
        assert bits_equal(xd, xs)
        A.free()


def test_add_f32(A):
    assert N_V4 > one_pass("ew_v4")
    a, b = tiled(torch.randn(PERIOD, generator=g(2)), N_V4), tiled(torch.randn(PERIOD - 2, generator=g(3)), N_V4)
    ad, bd, od = A.inp(a), A.inp(b), A.out((N_V4,), F32)
    ok(L().mv_add_f32(ptr(ad), ptr(bd), ptr(od), N_V4, stream()))
    A.check()
    assert bits_equal(od, a + b)


def _quant_float_input():
    gg = g(7)
    base = torch.randn(PERIOD, generator=gg) * torch.exp(torch.randn(PERIOD, generator=gg) * 5)
    base[:8] = torch.tensor([0.0, -0.0, 65504.0, 65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, -2.0 ** -26])
    return base


@pytest.mark.parametrize("e,m", [(5, 10), (4, 3)])
def test_quant_float(A, e, m):
    assert N_V4 > one_pass("ew_v4")
    base = _quant_float_input()
    want = tiled(torch.from_numpy(quant_oracle.float_quantize(base.numpy(), e, m)), N_V4)
    xd, yd = A.inp(tiled(base, N_V4)), A.out((N_V4,), F32)
    ok(L().mv_quant_float(ptr(xd), ptr(yd), N_V4, e, m, stream()))
    A.check()
    assert bits_equal(yd, want)


def test_quant_float_f16(A):
    assert N_V4 > one_pass("ew_v4")
    base = _quant_float_input()
    q = torch.from_numpy(quant_oracle.float_quantize(base.numpy(), 5, 10))
    assert torch.equal(q.half().float(), q)                      # every value of the format is a half: the conversion is exact
    xd, yd = A.inp(tiled(base, N_V4)), A.out((N_V4,), F16)
    ok(L().mv_quant_float_f16(ptr(xd), ptr(yd), N_V4, stream()))
    A.check()
    assert bits_equal(yd, tiled(q.half(), N_V4))


SEED, OFFSET = (5 << 40) + 12345, (3 << 32) + 7                   # bits in both 32-bit halves of the key and of the counter's high words


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_dropout_mask_and_kept_values(A, dtype, p):
    assert N_V4 > one_pass("ew_v4")
    x = tiled(torch.randn(PERIOD, generator=g(4)), N_V4).to(dtype)
    assert not bool((x == 0).any())                               # so a zero in the output is a dropped element
    keep = torch.from_numpy(dropout_keep_mask(N_V4, p, SEED, OFFSET))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(p))   # in float32, as mv_dropout computes it
    want = torch.where(keep, x.float() * float(scale), torch.zeros(())).to(dtype)
    xd, yd = A.inp(x), A.out((N_V4,), dtype)
    ok(L().mv_dropout(ptr(xd), ptr(yd), DT[dtype], N_V4, p, SEED, OFFSET, stream()))
    A.check()
    got = yd.cpu()
    assert torch.equal(got != 0, keep)
    assert bits_equal(got, want)
    assert abs(float(keep.float().mean()) - (1 - p)) < 5e-3


# ================================================================== 2. exact elementwise, one element per thread
def test_quant_fixed_and_affine(A):
    assert N_S1 > one_pass("ew_s1")
    base = torch.randn(PERIOD, generator=g(8)) * 3
    xd = A.inp(tiled(base, N_S1))
    for wl, fl in [(11, 8), (8, 4)]:
        yd = A.out((N_S1,), F32)
        ok(L().mv_quant_fixed(ptr(xd), ptr(yd), N_S1, wl, fl, 1, 0, stream()))
        A.check()
        assert bits_equal(yd, tiled(torch.from_numpy(quant_oracle.fixed_point_quantize(base.numpy(), wl, fl)), N_S1)), (wl, fl)
    s, z = quant_oracle.affine_qparams(float(base.min()), float(base.max()), 0, 255, False)
    yd = A.out((N_S1,), F32)
    ok(L().mv_quant_affine(ptr(xd), ptr(yd), N_S1, float(s), z, 0, 255, stream()))
    A.check()
    assert bits_equal(yd, tiled(torch.from_numpy(quant_oracle.fake_quant_affine(base.numpy(), s, z, 0, 255)), N_S1))


def test_minmax_extremes_in_the_second_pass_and_in_the_tail(A):
    assert N_S1 > one_pass("ew_s1")
    x = tiled(torch.randn(PERIOD, generator=g(9)), N_S1).clone()
    lo, hi = one_pass("ew_s1") + 700, N_S1 - 2                   # inside the second pass; among the last three elements
    x[lo], x[hi] = -100.0, 100.0
    assert float(x.min()) == -100.0 and float(x.max()) == 100.0
    xd = A.inp(x)
    inf = float("inf")
    # (state before) -> (state after): the state's own minimum beats the planted one, then its own maximum does
    for before, after in [((-1000.0, -inf), (-1000.0, 100.0)), ((inf, 1000.0), (-100.0, 1000.0)), ((inf, -inf), (-100.0, 100.0))]:
        st = A.inp(torch.tensor([before[0], before[1], 0.0, 0.0]))
        ok(L().mv_minmax(ptr(xd), N_S1, ptr(st), stream()))
        A.check()
        assert tuple(st[:2].tolist()) == after, (before, st.tolist())


# ================================================================== 3. GELU
def test_gelu_fp32(A):
    assert N_S1 > one_pass("ew_s1")
    hb, db = torch.randn(PERIOD, generator=g(10)) * 2, torch.randn(PERIOD, generator=g(11))
    h, dy = A.inp(tiled(hb, N_S1)), A.inp(tiled(db, N_S1))
    y, dx = A.out((N_S1,), F32), A.out((N_S1,), F32)
    ok(L().mv_gelu_fwd(ptr(h), ptr(y), MV_F32, N_S1, stream()))
    ok(L().mv_gelu_bwd(ptr(h), ptr(dy), ptr(dx), MV_F32, N_S1, stream()))
    A.check()
    # the bars of tests/test_hip_ops.py::test_cast_weightprep_gelu_add: 1e-6 forward, 2e-6 backward
    e_f, e_b = relerr(y, tiled(gelu_erf(hb.double()), N_S1)), relerr(dx, tiled(db.double() * dgelu64(hb), N_S1))
    print(f"gelu fp32: forward {e_f:.2e}, backward {e_b:.2e}")
    assert e_f < 1e-6 and e_b < 2e-6


def test_gelu_bf16(A):
    assert N_S1 > one_pass("ew_s1")
    hb, db = (torch.randn(PERIOD, generator=g(12)) * 2).to(BF16), torch.randn(PERIOD, generator=g(13)).to(BF16)
    h, dy = A.inp(tiled(hb, N_S1)), A.inp(tiled(db, N_S1))
    y, dx = A.out((N_S1,), BF16), A.out((N_S1,), BF16)
    ok(L().mv_gelu_fwd(ptr(h), ptr(y), MV_BF16, N_S1, stream()))
    ok(L().mv_gelu_bwd(ptr(h), ptr(dy), ptr(dx), MV_BF16, N_S1, stream()))
    A.check()
    # bf16 inputs against the fp64 value of those same inputs: the project's bf16-output bar, 2^-8 (tests/test_hip_ops.py)
    e_f, e_b = relerr(y, tiled(gelu_erf(hb.double()), N_S1)), relerr(dx, tiled(db.double() * dgelu64(hb), N_S1))
    print(f"gelu bf16: forward {e_f:.2e}, backward {e_b:.2e}")
    assert e_f < 2.0 ** -8 and e_b < 2.0 ** -8


# ================================================================== 4. integer codes
def _code_input(rows, cols, dtype, seed):
    base = ((torch.rand(PERIOD, generator=g(seed)) * 2 - 1) * 6).to(dtype)
    return tiled(base, rows * cols).view(rows, cols)


def _gelu_on_device(A, x):
    """mv_gelu_fwd in fp32 of a (bf16 or fp32) tensor's values: the unfused GELU that pre_op = 1 is held against."""
    xf, y = A.inp(x.float()), A.out(x.shape, F32)
    ok(L().mv_gelu_fwd(ptr(xf), ptr(y), MV_F32, x.numel(), stream()))
    A.check()
    return y


def _codes_against_reference(got, x, A, pre_op, shift, what):
    """got: integer codes [rows, cols] as float.  pre_op 0: exactly round(fake_quantize(x) / scale) (+ shift).  pre_op 1: the bar of
    tests/test_hip_ops.py for the GELU pre-op -- the kernel quantises a 1.5e-7-accurate GELU, the reference the exact one (mv_gelu_fwd,
    then the same quantiser): no code moves by more than one, fewer than 2e-4 of them move."""
    if pre_op == 0:
        assert torch.equal(got, affine_codes_ref(x, Q_SCALE, Q_ZERO) + shift), what
        return
    want = affine_codes_ref(_gelu_on_device(A, x).cpu(), Q_SCALE, Q_ZERO) + shift
    diff = (got - want).abs()
    moved = float((diff != 0).float().mean())
    print(f"{what}: {moved:.2e} of the codes moved by one")
    assert float(diff.max()) <= 1.0 and moved < 2e-4, what


@pytest.mark.parametrize("pre_op", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld,kernel", [(4101, 255, 257, "ew_s1"), (65541, 8, 12, "codes_vec")], ids=["generic", "vector"])
def test_quant_affine_codes(A, rows, cols, ld, kernel, dtype, pre_op):
    assert (rows * ld if kernel == "ew_s1" else rows) > one_pass(kernel)
    x = _code_input(rows, cols, dtype, 20)
    xd, yd = A.inp(x), A.out((rows, ld), BF16)
    ok(L().mv_quant_affine_codes(ptr(xd), DT[dtype], ptr(yd), rows, cols, ld, Q_SCALE, Q_ZERO, 0, 255, pre_op, stream()))
    A.check()
    got = yd.cpu().float()
    assert not bool(got[:, cols:].any())                                    # padding columns are zero
    _codes_against_reference(got[:, :cols], x, A, pre_op, 0.0, f"codes {kernel} {dtype} pre_op {pre_op}")


@pytest.mark.parametrize("pre_op", [0, 1])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld,kernel", [(4101, 40, 48, "i8_rows"), (16389, 1024, 1024, "ew_w4")], ids=["rows", "flat"])
def test_quant_affine_i8(A, rows, cols, ld, kernel, dtype, pre_op):
    assert (rows if kernel == "i8_rows" else rows * cols // 1024) > one_pass(kernel)      # a wave of the flat form takes 1024 elements
    x = _code_input(rows, cols, dtype, 21)
    xd, yd = A.inp(x), A.out((rows, ld), I8)
    ok(L().mv_quant_affine_i8(ptr(xd), DT[dtype], ptr(yd), rows, cols, ld, Q_SCALE, Q_ZERO, pre_op, stream()))
    A.check()                                                               # no operand is 0x7f: level 255 is out of the inputs' reach
    got = yd.cpu().float()
    assert not bool(got[:, cols:].any())
    # q - 128 with q the uint8 level (tests/test_hip_ops.py::test_int8_mfma_gemm_is_the_exact_integer_product)
    _codes_against_reference(got[:, :cols], x, A, pre_op, float(Q_ZERO - 128), f"i8 {kernel} {dtype} pre_op {pre_op}")
    assert float(got.max()) < 127.0 and (pre_op == 1 or float(got.min()) == -128.0)   # the pre-fill value never; the low clamp without GELU


# ================================================================== 5. layout kernels
@pytest.mark.parametrize("B,C,H,W,p,items", [(84, 3, 224, 224, 16, 84 * 224 * 56), (700, 1, 32, 48, 8, 700 * 32 * 48)], ids=["rgb", "generic"])
def test_patchify(A, B, C, H, W, p, items):
    assert items > one_pass("ew_s1")
    img = torch.randn(B, C, H, W, generator=g(30))
    want = patchify_oracle(img, p).reshape(-1, p * p * C)
    imd = A.inp(img)
    for dtype in (F32, BF16):
        od = A.out(want.shape, dtype)
        ok(L().mv_patchify(ptr(imd), ptr(od), DT[dtype], B, C, H, W, p, stream()))
        A.check()
        assert bits_equal(od, want.to(dtype)), dtype
    assert bits_equal(imd, img)


def test_embed_cls_changes_row_zero_only(A):
    B, T, D = 1367, 2, 768
    assert B * D > one_pass("ew_s1")
    cls, pos = torch.randn(D, generator=g(31)), torch.randn(T, D, generator=g(32))
    x = torch.randn(B, T, D, generator=g(33))
    cd, pd, xd = A.inp(cls), A.inp(pos), A.inp(x)
    ok(L().mv_embed_cls(ptr(cd), ptr(pd), ptr(xd), B, T, D, stream()))
    A.check()
    want = x.clone()
    want[:, 0] = cls + pos[0]
    assert bits_equal(xd, want)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
def test_gather_patch_rows(A, dtype):
    B, T, D = 3, 1367, 1024
    assert B * (T - 1) * (D // 4) > one_pass("ew_s1")
    src = torch.randn(B, T, D, generator=g(34))
    sd, od = A.inp(src), A.out((B * (T - 1), D), dtype)
    ok(L().mv_gather_patch_rows(ptr(sd), ptr(od), DT[dtype], B, T, D, stream()))
    A.check()
    assert bits_equal(od, src[:, 1:].reshape(-1, D).to(dtype))


@pytest.mark.parametrize("role", [0, 1])
@pytest.mark.parametrize("nseg", [6, 3], ids=["split3", "split2"])
def test_split_pieces(A, nseg, role):
    """The restatement of tests/test_hip_ops.py::test_split3_bf16_pieces_reconstruct_fp32 on every element: the segments hold the
    pieces in the documented order, equal pieces are equal bits, piece 0 is bf16(x), and the pieces sum back to x to 2^-26 |x|
    (2^-17 |x| for the two pieces of split2) -- and each piece is the one the fp32 piece arithmetic gives."""
    rows, cols, ldx = 4101, 1024, 1028
    assert rows * (cols // 4) > one_pass("ew_s1")
    x = (torch.randn(rows, ldx, generator=g(35)) * torch.logspace(-12, 12, ldx))
    xd, od = A.inp(x), A.out((rows, nseg * cols), BF16)
    fn = L().mv_split3_bf16 if nseg == 6 else L().mv_split2_bf16
    ok(fn(ptr(xd), ldx, ptr(od), nseg * cols, cols, rows, cols, role, stream()))
    A.check()
    segs = od.cpu().view(rows, nseg, cols)
    want = split_pieces(x[:, :cols])
    held = {}
    for s_, pi in enumerate(SPLIT_ORDER[role][:nseg]):
        held.setdefault(pi, segs[:, s_])
        assert bits_equal(segs[:, s_], held[pi]) and bits_equal(segs[:, s_], want[pi]), (s_, pi)
    xr = x[:, :cols].double()
    total = sum(v.double() for v in held.values())
    assert bool(((total - xr).abs() <= xr.abs() * (2.0 ** -26 if nseg == 6 else 2.0 ** -17)).all())


# ================================================================== 6. reductions on integer-valued inputs
def exact_in_fp32(*sums):
    """The condition on the inputs: every partial sum a kernel can form is an integer below 2^24 (it is at most the sum of the
    magnitudes), so any summation order gives the same fp32 bits."""
    return all(int(s.abs().max()) < 2 ** 24 for s in sums)


@pytest.mark.parametrize("S", [1, 3])
def test_sum_slabs(A, S):
    n, stride = N_V4, N_V4 + 9                                              # slabs further apart than they are long
    assert n > one_pass("ew_v4") and stride % 4 == 0
    slabs = small_ints((S, stride), 40 + S)
    prior, add = small_ints((n,), 43), small_ints((n,), 44)
    total = slabs[:, :n].to(I64).sum(0)
    assert exact_in_fp32(slabs[:, :n].to(I64).abs().sum(0) + prior.to(I64).abs() + add.to(I64).abs())
    sd = A.inp(slabs)
    for accumulate in (0, 1):
        od = A.inp(prior) if accumulate else A.out((n,), F32)
        ok(L().mv_sum_slabs(ptr(sd), stride, S, ptr(od), n, accumulate, stream()))
        A.check()
        assert bits_equal(od, (total + (prior.to(I64) if accumulate else 0)).float()), accumulate
    od = A.inp(add)                                                         # add aliases out
    ok(L().mv_sum_slabs_add(ptr(sd), stride, S, ptr(od), ptr(od), n, stream()))
    A.check()
    assert bits_equal(od, (total + add.to(I64)).float())
    ad, od = A.inp(add), A.out((n,), F32)                                   # add distinct from out
    ok(L().mv_sum_slabs_add(ptr(sd), stride, S, ptr(ad), ptr(od), n, stream()))
    A.check()
    assert bits_equal(od, (total + add.to(I64)).float()) and bits_equal(ad, add) and bits_equal(sd, slabs)


def test_embed_bwd(A):
    B, T, D = 3, 1367, 768
    assert T * D > one_pass("ew_s1")
    dx = small_ints((B, T, D), 45)
    prior_pos, prior_cls = small_ints((T, D), 46), small_ints((D,), 47)
    total = dx.to(I64).sum(0)
    assert exact_in_fp32(dx.to(I64).abs().sum(0) + prior_pos.to(I64).abs())
    xd = A.inp(dx)
    for accumulate in (0, 1):
        dpos = A.inp(prior_pos) if accumulate else A.out((T, D), F32)
        dcls = A.inp(prior_cls) if accumulate else A.out((D,), F32)
        ok(L().mv_embed_bwd(ptr(xd), ptr(dpos), ptr(dcls), accumulate, B, T, D, stream()))
        A.check()
        assert bits_equal(dpos, (total + (prior_pos.to(I64) if accumulate else 0)).float()), accumulate
        assert bits_equal(dcls, (total[0] + (prior_cls.to(I64) if accumulate else 0)).float()), accumulate


COLSUM_ROWS = [1, 5, 2048, 2049, 65536, 65541]      # one-stage (fp32, rows <= 2048) | two-stage | the 256-part cap and past it
COLSUM_WIDTHS = [(45, 48), (46, 46), (768, 768), (1000, 1004)]   # vector + scalar last group | scalar (ld % 4) | vector | vector, padded


@pytest.mark.parametrize("cols,ld", COLSUM_WIDTHS)
@pytest.mark.parametrize("rows", COLSUM_ROWS)
def test_colsum_direct(A, rows, cols, ld):
    parts = min(max((rows + 255) // 256, 1), 256)
    if rows > 65536:
        assert parts == 256 and rows > one_pass("colsum_parts")
    x = small_ints((rows, ld), 50 + rows % 7 + cols, torch.int8)
    prior = small_ints((cols,), 51)
    total = x[:, :cols].sum(0, dtype=I64)
    assert exact_in_fp32(x[:, :cols].abs().sum(0, dtype=I64) + prior.to(I64).abs())
    nbytes = parts * cols * 4
    for dtype in (F32, BF16):
        xd = A.inp(x.to(dtype))
        for accumulate in (0, 1):
            od, ws = A.inp(prior) if accumulate else A.out((cols,), F32), A.scratch(nbytes)
            ok(L().mv_colsum(ptr(xd), DT[dtype], ld, ptr(od), accumulate, rows, cols, ptr(ws), nbytes, stream()))
            A.check()
            assert bits_equal(od, (total + (prior.to(I64) if accumulate else 0)).float()), (dtype, accumulate)
        A.free()


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("max_norm", [100.0, 1.0e4], ids=["clips", "passes"])
def test_grad_norm_clip(A, max_norm, grad_scale):
    n = N_SUMSQ
    assert n > one_pass("sumsq")
    gr = small_ints((n,), 52)
    S, total, coef = grad_norm_ref(gr, grad_scale, max_norm)
    assert S < 2 ** 53                                   # exact in fp64; a thread's fp32 partial is nine squares of at most 64
    nbytes = L().mv_grad_norm_workspace_bytes()
    gd, od, ws = A.inp(gr), A.out((2,), F32), A.scratch(nbytes)
    ok(L().mv_grad_norm_clip(ptr(gd), n, grad_scale, max_norm, ptr(od), ptr(ws), nbytes, stream()))
    A.check()
    got_total, got_coef = (np.float32(v) for v in od.tolist())
    print(f"grad norm: total {got_total!r} want {total!r}; coefficient {got_coef!r}")
    assert abs(float(got_total) - float(total)) <= float(np.spacing(total))          # one fp32 ulp: the device's double square root
    assert got_coef == coef(got_total)
    assert (got_coef < 1.0) == (max_norm == 100.0)
    assert bits_equal(gd, gr)


# ================================================================== 7. row kernels, one wave per row
SOFTMAX_COLS = [17, 64, 197, 257]


def _softmax64(x, scale):
    return torch.softmax(x.double() * float(np.float32(scale)), dim=1)


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_fwd(A, cols):
    rows, scale = R_W4, 0.125
    assert rows > one_pass("softmax")
    x = torch.randn(rows, cols, generator=g(60)) * 8
    xd, yd = A.inp(x), A.out((rows, cols), F32)
    ok(L().mv_softmax_fwd(ptr(xd), ptr(yd), rows, cols, scale, stream()))
    A.check()
    e = relerr(yd, _softmax64(x, scale))
    print(f"softmax forward cols={cols}: {e:.2e}")
    assert e < 5e-6                                     # the bar of tests/test_hip_ops.py::test_attention_materialised_fp32


@pytest.mark.parametrize("cols", SOFTMAX_COLS)
def test_softmax_bwd(A, cols):
    """dx = scale * y * (dy - sum(y * dy)) against the fp64 value of the formula on the same fp32 y and dy.  No project bar exists
    for this call; the bar is 8 x the max-normalised error of a plain fp32 torch evaluation on the CPU against the same fp64 value.
    Measured on an MI355X (cols 17 / 64 / 197 / 257): fp32 torch 1.22e-07 / 9.40e-08 / 5.51e-08 / 5.66e-08; the kernel
    1.02e-07 / 9.13e-08 / 7.64e-08 / 4.61e-08 -- at most 1.4 x the reference's error, against the 8 x allowed."""
    rows, scale = R_W4, 0.125
    assert rows > one_pass("softmax")
    y = _softmax64(torch.randn(rows, cols, generator=g(61)) * 8, scale).float()
    dy = torch.randn(rows, cols, generator=g(62))
    s32 = float(np.float32(scale))
    want = s32 * y.double() * (dy.double() - (y.double() * dy.double()).sum(1, keepdim=True))
    plain = np.float32(scale) * y * (dy - (y * dy).sum(1, keepdim=True))
    base = relerr(plain, want)
    yd, dd, od = A.inp(y), A.inp(dy), A.out((rows, cols), F32)
    ok(L().mv_softmax_bwd(ptr(yd), ptr(dd), ptr(od), rows, cols, scale, stream()))
    A.check()
    e = relerr(od, want)
    print(f"softmax backward cols={cols}: fp32 torch {base:.2e}, bound {8 * base:.2e}, kernel {e:.2e}")
    assert e <= 8 * base


def _ce_reference(logits, labels):
    ref = logits.double().requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(ref, labels)
    loss.backward()
    return float(loss.detach()), ref.grad


def _run_ce(A, logits, labels, outer, C, inner, dl_dtype, ld_dl):
    ld, lb = A.inp(logits), A.inp(labels)
    stat = A.out((4,), F32)
    dl = A.out((outer, ld_dl) if inner == 1 else logits.shape, dl_dtype)
    am = A.out(labels.shape, I64)
    ok(L().mv_cross_entropy(ptr(ld), ptr(lb), ptr(stat), ptr(dl), DT[dl_dtype], ld_dl, ptr(am), outer, C, inner, 1.0, stream()))
    A.check()
    return float(stat[0]), dl.cpu(), am.cpu(), float(stat[1])


@pytest.mark.parametrize("C", [45, 130])
def test_cross_entropy_one_wave_per_sample(A, C):
    B = R_W4
    assert B > one_pass("ew_w4")
    logits = torch.randn(B, C, generator=g(63)) * 3
    labels = torch.randint(0, C, (B,), generator=g(64))
    labels[::97] = -100                                                   # ignored: first pass, second pass and the last sample
    labels[-1] = -100
    want, want_grad = _ce_reference(logits, labels)
    loss, dl, am, counted = _run_ce(A, logits, labels, B, C, 1, F32, C)
    # the bars of tests/test_hip_ops.py::test_cross_entropy_cls: 1e-5, 1e-5, 2^-8, exact
    print(f"cross entropy C={C}: loss {loss:.8f} ref {want:.8f}; gradient {relerr(dl, want_grad):.2e}")
    assert counted == float((labels != -100).sum())
    assert abs(loss - want) < 1e-5 * max(1, abs(want))
    assert relerr(dl, want_grad) < 1e-5
    assert torch.equal(am, logits.argmax(1))
    assert not bool(dl[labels == -100].any())
    ldp = (C + 7) & ~7
    _, dlp, _, _ = _run_ce(A, logits, labels, B, C, 1, BF16, ldp)
    assert dlp.shape == (B, ldp) and not bool(dlp[:, C:].any())
    assert relerr(dlp[:, :C].float(), want_grad) < 2.0 ** -8


def test_cross_entropy_one_thread_per_pixel(A):
    B, C, S = 2, 5, 725
    assert B * S * S > one_pass("ew_s1")
    logits = torch.randn(B, C, S, S, generator=g(65)) * 2
    labels = torch.randint(0, C, (B, S, S), generator=g(66))
    labels[0, :3] = -100
    labels[1, -1, -5:] = -100                                             # the last pixels of the second pass
    want, want_grad = _ce_reference(logits, labels)
    for dtype, bar in ((F32, 1e-5), (BF16, 2.0 ** -8)):
        loss, dl, am, counted = _run_ce(A, logits, labels, B, C, S * S, dtype, C)
        print(f"pixel cross entropy {dtype}: loss {loss:.8f} ref {want:.8f}; gradient {relerr(dl.float(), want_grad):.2e}")
        assert counted == float((labels != -100).sum())
        assert abs(loss - want) < 1e-5 * abs(want)                        # tests/test_hip_ops.py::test_cross_entropy_seg
        assert relerr(dl.float(), want_grad) < bar
        assert torch.equal(am, logits.argmax(1))
        assert not bool(dl.permute(0, 2, 3, 1)[labels == -100].any())
        A.free()


@pytest.mark.parametrize("lam,eps", [(1.0, 0.0), (0.3, 0.1)])
@pytest.mark.parametrize("C", [5, 37])
def test_cross_entropy_soft(A, C, lam, eps):
    """The bars of tests/test_mixup_gpu.py::test_soft_cross_entropy_against_fp64 (TOL = 1e-5): mean loss, per-sample losses,
    relative L2 of the gradient, arg-max equal to torch's."""
    B, TOL = R_W4, 1e-5
    assert B > one_pass("ce_soft")
    gg = g(7 * B + C)
    logits, labels = torch.randn(B, C, generator=gg) * 3, torch.randint(0, C, (B,), generator=gg)
    z = logits.double().requires_grad_()
    t = soft_target(labels, C, lam, eps)
    want_per = torch.nn.functional.cross_entropy(z, t, reduction="none").detach()
    mean = torch.nn.functional.cross_entropy(z, t)
    mean.backward()
    want = float(mean)
    ld, lb = A.inp(logits), A.inp(labels)
    loss, per, dl, am = A.out((1,), F32), A.out((B,), F32), A.out((B, C), F32), A.out((B,), I64)
    ok(L().mv_cross_entropy_soft(ptr(ld), ptr(lb), ptr(loss), ptr(per), ptr(dl), ptr(am), B, C, lam, eps, 1, 1.0, stream()))
    A.check()
    e_per = float(((per.double().cpu() - want_per).abs() / want_per.abs().clamp_min(1.0)).max())
    e_grad = float((dl.double().cpu() - z.grad).norm() / z.grad.norm())
    print(f"soft cross entropy C={C} lam={lam} eps={eps}: loss {float(loss):.8f} ref {want:.8f}; per-sample {e_per:.2e}; dlogits {e_grad:.2e}")
    assert abs(float(loss) - want) < TOL * max(1.0, abs(want))
    assert e_per < TOL and e_grad < TOL
    assert torch.equal(am.cpu(), logits.argmax(1))


@pytest.mark.parametrize("mode", ["soft", "hard"])
@pytest.mark.parametrize("C", [5, 37])
def test_distill_loss(A, C, mode):
    """The rule of tests/test_distill_gpu.py: each quantity within 8 x the largest error of torch's own fp32 evaluation against
    the fp64 oracle (distill_ref.baselines, computed when the tests run)."""
    B = R_W4
    assert B > one_pass("distill")
    s, d, t, y = distill_ref.inputs(B, C)
    base = distill_ref.baselines()
    sd, dd_, td, yd = A.inp(s), A.inp(d), A.inp(t), A.inp(y)
    for T, alpha, (lam, eps, flip) in [(1.0, 0.5, (1.0, 0.0, False)), (3.0, 0.5, (0.3, 0.1, True))]:
        ref = distill_ref.oracle(s.numpy(), d.numpy(), t.numpy(), y.numpy(), T, alpha, mode, lam, eps, flip)
        loss, per = A.out((3,), F32), A.out((2, B), F32)
        ds, dd, am = A.out((B, C), F32), A.out((B, C), F32), A.out((B,), I64)
        ok(L().mv_distill_loss(ptr(sd), ptr(dd_), ptr(td), ptr(yd), ptr(loss), ptr(per), ptr(ds), ptr(dd), ptr(am), B, C,
                               {"soft": 0, "hard": 1}[mode], T, alpha, lam, eps, int(flip), 1.0, stream()))
        A.check()
        lv = loss.cpu().double().numpy()
        got = dict(loss=lv[0], ce=lv[1], kd=lv[2], dstudent=ds.cpu().numpy(), ddistill=dd.cpu().numpy())
        for k in distill_ref.QUANTITIES:
            e = distill_ref.rel_err(got[k], ref[k])
            print(f"distill C={C} {mode} T={T}: {k} kernel {e:.3e} bound {distill_ref.FACTOR * base[k]:.3e}")
            assert e <= distill_ref.FACTOR * base[k], (k, e, base[k])
        assert torch.equal(am.cpu(), s.argmax(1))
    assert bits_equal(td, t)


def _upsample_reference(small_cf, size, dbig):
    ref = small_cf.double().requires_grad_(True)
    want = torch.nn.functional.interpolate(ref, size=(size, size), mode="bilinear", align_corners=False)
    want.backward(dbig.double())
    return want.detach(), ref.grad


def test_upsample_bilinear_fwd(A):
    B, C, h, H = 2, 3, 14, 420
    assert B * C * H * H > one_pass("ew_s1")
    small = torch.randn(B, C, h, h, generator=g(70))                      # channels first; the channels-last copy holds the same values
    want, _ = _upsample_reference(small, H, torch.zeros(B, C, H, H))
    for name, data, (sb, sc, sp) in [("channels first", small, (C * h * h, h * h, 1)),
                                     ("channels last", small.permute(0, 2, 3, 1).contiguous(), (h * h * C, 1, C))]:
        sd, bd = A.inp(data), A.out((B, C, H, H), F32)
        ok(L().mv_upsample_bilinear_fwd(ptr(sd), sb, sc, sp, ptr(bd), B, C, h, h, H, H, stream()))
        A.check()
        e = relerr(bd, want)
        print(f"upsample forward, {name}: {e:.2e}")
        assert e < 2e-6                                                   # tests/test_hip_ops.py::test_upsample_bilinear


def test_upsample_bilinear_bwd(A):
    B, C, h, H = 2, 33, 128, 256
    assert B * C * h * h > one_pass("ew_s1")
    dbig = torch.randn(B, C, H, H, generator=g(71))
    _, want = _upsample_reference(torch.zeros(B, C, h, h), H, dbig)
    dd = A.inp(dbig)
    for name, shape, (sb, sc, sp), back in [("channels first", (B, C, h, h), (C * h * h, h * h, 1), lambda v: v),
                                            ("channels last", (B, h, h, C), (h * h * C, 1, C), lambda v: v.permute(0, 3, 1, 2))]:
        sd = A.out(shape, F32)
        ok(L().mv_upsample_bilinear_bwd(ptr(dd), ptr(sd), sb, sc, sp, B, C, h, h, H, H, stream()))
        A.check()
        e = relerr(back(sd.cpu()), want)
        print(f"upsample backward, {name}: {e:.2e}")
        assert e < 5e-6                                                   # tests/test_hip_ops.py::test_upsample_bilinear


# ================================================================== 8. LayerNorm forward
EPS = 1e-5


def _ln_params(dim):
    return (torch.randn(dim, generator=g(81)) * 0.1 + 1), torch.randn(dim, generator=g(82)) * 0.1


def _ln_reference(x, gam, bet):
    """-> (y, mean, rstd) in fp64, and the max-normalised errors of the plain fp32 torch evaluation of mean and rstd against them."""
    xd = x.double()
    mu = xd.mean(1)
    rstd = 1.0 / torch.sqrt(((xd - mu[:, None]) ** 2).mean(1) + EPS)
    mu32 = x.mean(1)
    rstd32 = 1.0 / torch.sqrt(((x - mu32[:, None]) ** 2).mean(1) + EPS)
    return ln_oracle(xd, gam.double(), bet.double(), EPS), mu, rstd, relerr(mu32, mu), relerr(rstd32, rstd)


def _run_ln(A, xd, gd, bd, rows, dim, dtype):
    y, mean, rstd = A.out((rows, dim), dtype), A.out((rows,), F32), A.out((rows,), F32)
    ok(L().mv_layernorm_fwd(ptr(xd), dim, ptr(gd), ptr(bd), ptr(y), DT[dtype], ptr(mean), ptr(rstd), rows, dim, EPS, stream()))
    A.check()
    return y, mean, rstd


Y_BAR = {F32: 2e-6, BF16: 2.0 ** -8}                  # tests/test_hip_ops.py::test_layernorm_fwd_bwd


@pytest.mark.parametrize("dim", [384, 512, 1028, 2048, 2052, 4096])      # width classes 2, 8 and 16 at both of their ends
@pytest.mark.parametrize("rows", [5, 394])
def test_layernorm_fwd_width_classes(A, rows, dim):
    """y against oracle.vit_oracle.layer_norm in fp64 at the existing bars; mean and rstd against fp64 at 8 x the error of a plain
    fp32 torch evaluation on the CPU.  Measured on an MI355X over these twelve shapes: fp32 torch mean 5.8e-08 .. 1.5e-07, rstd
    4.3e-08 .. 1.4e-07; the kernel mean 5.3e-08 .. 1.4e-07, rstd 1.9e-08 .. 1.1e-07 -- at most 1.3 x the reference's error in any
    one shape, against the 8 x allowed."""
    x = torch.randn(rows, dim, generator=g(80)) * 2 + 0.5
    gam, bet = _ln_params(dim)
    want, mu, rs, base_mu, base_rs = _ln_reference(x, gam, bet)
    xd, gd, bd = A.inp(x), A.inp(gam), A.inp(bet)
    for dtype in (F32, BF16):
        y, mean, rstd = _run_ln(A, xd, gd, bd, rows, dim, dtype)
        e_y, e_mu, e_rs = relerr(y.float(), want), relerr(mean, mu), relerr(rstd, rs)
        print(f"layernorm {rows}x{dim} {dtype}: y {e_y:.2e}; mean fp32 torch {base_mu:.2e} kernel {e_mu:.2e}; "
              f"rstd fp32 torch {base_rs:.2e} kernel {e_rs:.2e}")
        assert e_y < Y_BAR[dtype]
        assert e_mu <= 8 * base_mu and e_rs <= 8 * base_rs


LN_PERIOD = 61


def _periodic_rows(base, rows):
    return base.cuda()[torch.arange(rows, device="cuda") % base.shape[0]]


def _worst_against_period(got, want, chunk=LN_PERIOD * 16):
    """max over every row of |got - its period's reference|, normalised by max|reference|; on the device, a slab of rows at a time."""
    want = want.cuda()
    worst = 0.0
    for r0 in range(0, got.shape[0], chunk):
        part = got[r0:r0 + chunk].double()
        ref = want.repeat(chunk // LN_PERIOD, *([1] * (want.dim() - 1)))[:part.shape[0]]
        worst = max(worst, float((part - ref).abs().max()))
    return worst / float(want.abs().max())


@pytest.mark.parametrize("dim", [64, 384, 768, 1000, 2048, 4096])
def test_layernorm_fwd_past_one_pass(A, dim):
    """Rows repeat with period 61, so the fp64 reference is 61 rows; every output row is held to its period's reference at the bars
    above, and rows 61 apart are bit-identical: a second-pass row runs the same code on the same data as a first-pass row."""
    rows = R_LN
    assert rows > one_pass("ln_fwd")
    base = torch.randn(LN_PERIOD, dim, generator=g(83)) * 2 + 0.5
    gam, bet = _ln_params(dim)
    want, mu, rs, base_mu, base_rs = _ln_reference(base, gam, bet)
    xd, gd, bd = A.inp(_periodic_rows(base, rows)), A.inp(gam), A.inp(bet)
    for dtype in (F32, BF16):
        y, mean, rstd = _run_ln(A, xd, gd, bd, rows, dim, dtype)
        view = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(y.view(view)[LN_PERIOD:], y.view(view)[:-LN_PERIOD]), dtype
        assert torch.equal(mean.view(torch.int32)[LN_PERIOD:], mean.view(torch.int32)[:-LN_PERIOD])
        assert torch.equal(rstd.view(torch.int32)[LN_PERIOD:], rstd.view(torch.int32)[:-LN_PERIOD])
        e_y, e_mu, e_rs = _worst_against_period(y, want), _worst_against_period(mean, mu), _worst_against_period(rstd, rs)
        print(f"layernorm {rows}x{dim} {dtype}: y {e_y:.2e}; mean {e_mu:.2e} of {8 * base_mu:.2e}; rstd {e_rs:.2e} of {8 * base_rs:.2e}")
        assert e_y < Y_BAR[dtype]
        assert e_mu <= 8 * base_mu and e_rs <= 8 * base_rs


@pytest.mark.parametrize("dim", [384, 768, 1000])
@pytest.mark.parametrize("nseg", [3, 6])
def test_layernorm_fwd_split_past_one_pass(A, nseg, dim):
    """Bit-equal to LayerNorm followed by the split pass, statistics included
    (tests/test_hip_ops.py::test_layernorm_fwd_split_equals_layernorm_then_split at small sizes)."""
    rows = R_LN
    assert rows > one_pass("ln_fwd")
    base = torch.randn(LN_PERIOD, dim, generator=g(84)) * 2 + 0.3
    gam, bet = _ln_params(dim)
    xd, gd, bd = A.inp(_periodic_rows(base, rows)), A.inp(gam), A.inp(bet)
    y, mean, rstd = _run_ln(A, xd, gd, bd, rows, dim, F32)
    want = A.out((rows, nseg * dim), BF16)
    split = L().mv_split3_bf16_ex if nseg == 6 else L().mv_split2_bf16_ex
    ok(split(ptr(y), dim, None, 0, 0, ptr(want), rows, dim, None, None, 0, stream()))
    A.check()
    got, m2, r2 = A.out((rows, nseg * dim), BF16), A.out((rows,), F32), A.out((rows,), F32)
    ok(L().mv_layernorm_fwd_split(ptr(xd), dim, ptr(gd), ptr(bd), ptr(got), nseg, ptr(m2), ptr(r2), rows, dim, EPS, stream()))
    A.check()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(m2.view(torch.int32), mean.view(torch.int32)) and torch.equal(r2.view(torch.int32), rstd.view(torch.int32))


@pytest.mark.parametrize("dim", [384, 768, 1024])
def test_layernorm_fwd_q8_past_one_pass(A, dim):
    """Bit-equal to LayerNorm followed by mv_quant_affine_i8 (tests/test_hip_ops.py::test_fused_quantiser_producers_are_bit_identical)."""
    rows = R_LN
    assert rows > one_pass("ln_fwd")
    base = torch.randn(LN_PERIOD, dim, generator=g(85)) * 2 + 0.5
    gam, bet = _ln_params(dim)
    xd, gd, bd = A.inp(_periodic_rows(base, rows)), A.inp(gam), A.inp(bet)
    y, _, _ = _run_ln(A, xd, gd, bd, rows, dim, F32)
    q_scale, q_zero = 0.04, 60                      # level 0 from y < -2.4 down; level 255, the pre-fill's operand, only from y > 7.8
    assert float(y.min()) < -2.5 and float(y.max()) < 7.7
    want, got = A.out((rows, dim), I8), A.out((rows, dim), I8)
    ok(L().mv_quant_affine_i8(ptr(y), MV_F32, ptr(want), rows, dim, dim, q_scale, q_zero, 0, stream()))
    ok(L().mv_layernorm_fwd_q8(ptr(xd), dim, ptr(gd), ptr(bd), ptr(got), rows, dim, EPS, q_scale, q_zero, stream()))
    A.check()
    assert torch.equal(got, want)
    assert int(want.max()) < 127 and int(want.min()) == -128
