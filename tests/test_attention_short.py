"""The whole-head attention kernels (N <= 320 bf16, <= 288 half operands, <= 272 fp32) at every dispatch and tile edge.

mv_attention_fwd / _bwd, mv_attention_fwd_f16 / _bwd_f16 and mv_attention_fwd_f32 / _f32_lse / _f32_q8 / mv_attention_bwd_f32
change kernel at 192 | 193, 208 | 209, 224 | 225 and 288 | 289, and tile at every multiple of 16.  Five groups of tests:

1. routing: inputs whose softmax is an exact permutation matrix, so which key reaches which query row is pinned bit for bit;
2. every edge and every variant against fp64: the whole-tensor ceilings of tests/test_hip_ops.py, a derived per-element forward
   bound, and -- on two harder score distributions -- a backward bar of 2x the error of an fp64 emulation of the kernel's roundings;
3. guard zones: every tensor in the middle of a larger allocation, NaN next to the inputs, sentinels round the outputs;
4. (image, head) independence, key permutation, zero gradient;
5. the API edges that launch nothing.

The input builders and the emulation are plain CPU torch; their preconditions are the unmarked tests at the top."""
import math
from contextlib import contextmanager

import pytest
import torch

gpu = pytest.mark.gpu

SCALE = 64 ** -0.5
EDGES = [1, 15, 16, 17, 192, 193, 197, 207, 208, 209, 223, 224, 225, 256, 257, 271, 272, 273, 287, 288, 289, 304, 319, 320]
CAP = {"bf16": 320, "half": 288, "fp32": 272}
GUARD_N = [1, 17, 197, 209, 225, 289, 320]
FAMILIES = ("bf16", "half", "fp32")
MV_OK, MV_ERR_SHAPE, MV_ERR_ALIGN, MV_ERR_UNSUPPORTED = 0, -1, -2, -4
OPERAND = {"bf16": torch.bfloat16, "half": torch.float16, "fp32": torch.float32}
# whole-tensor ceilings of tests/test_hip_ops.py (max-norm relative error): forward, backward, lse (absolute)
CEIL = {"bf16": (1.5e-2, 3e-2, 1e-4), "half": (6e-4, 2e-3, 2e-5), "fp32": (2e-6, 5e-6, 2e-5)}
U_P = {"bf16": 2.0 ** -9, "half": 2.0 ** -12}      # unit roundoff of P
U_OUT = {"bf16": 2.0 ** -9, "half": 0.0}           # ... of the output (the half kernels write fp32)


def edges(family):
    return [n for n in EDGES if n <= CAP[family]]


def family_lengths(lengths):
    return [(f, n) for f in FAMILIES for n in lengths if n <= CAP[f]]


def bwd_variants(N):
    """mv_attention_bwd_force values whose kernel takes N (0 = automatic; 5 is the two-wave form only when N > 192)."""
    return [0] + [v for v, nmax in ((4, 208), (5, 208), (2, 288), (8, 320)) if N <= nmax]


FWD_VARIANTS = (0, 1, 2, 3)


def g(seed):
    return torch.Generator().manual_seed(seed)


def relmax(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def heads(x, H, dh=64):
    """[B, N, H * dh] -> [B, H, N, dh]"""
    B, N, _ = x.shape
    return x.view(B, N, H, dh).transpose(1, 2)


def unheads(x):
    """[B, H, N, dh] -> [B, N, H * dh]"""
    B, H, N, dh = x.shape
    return x.transpose(1, 2).reshape(B, N, H * dh)


def split_qkv(qkv, H, dh=64):
    """[B, N, 3 * H * dh] -> q, k, v, each [B, H, N, dh]"""
    B, N, _ = qkv.shape
    return qkv.view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)


def join_qkv(q, k, v):
    """q, k, v [B, H, N, dh] -> [B, N, 3 * H * dh]"""
    B, H, N, dh = q.shape
    return torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * dh).contiguous()


def bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


# ================================================================== builders (CPU)
# ---------------------------------------------------------------- routing: softmax = an exact permutation matrix
ROUTING_MULT = {64: 8.0, 32: 16.0, 128: 8.0}     # k = mult * r with r = +-1: exact in bf16 and half
ROUTING_MIN_GAP = {64: 128.0, 32: 104.0, 128: 104.0}   # score units; exp(-104) < 2^-149, the smallest fp32 subnormal
ROUTING_CASES = ([(64, n) for n in EDGES] + [(64, 577), (64, 1025)] + [(32, 197), (32, 577), (128, 197), (128, 577)])
# the key-tiled kernels called directly at their block edges (tests/test_attention_tiled.py)
TILED_EDGES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320, 321, 383, 384, 385, 511, 512, 513]
TILED_EDGES_DH = {32: [1, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513],      # 256 rows per workgroup
                  128: [1, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385]}
ROUTING_CASES += [(64, n) for n in TILED_EDGES if n not in EDGES] + [(dh, n) for dh in (32, 128) for n in TILED_EDGES_DH[dh]]


def routing_inputs(B, N, H, dh=64):
    """-> qkv [B, N, 3*H*dh], dout [B, N, H*dh] (fp32 holding values exact in bf16 and half), perm [B, H, N], r [B, H, N, dh].
    Keys are mult * r with r = +-1, query i is key perm[i]: its score with that key is mult^2 * dh * scale, every other score is
    mult^2 * scale * (r . r') -- at least ROUTING_MIN_GAP below.  v and dout are integers in [-8, 8]."""
    gen = g(1000 * dh + N)
    r = torch.randint(0, 2, (B, H, N, dh), generator=gen).float() * 2 - 1
    k = ROUTING_MULT[dh] * r
    perm = torch.stack([torch.stack([torch.randperm(N, generator=gen) for _ in range(H)]) for _ in range(B)])
    q = torch.gather(k, 2, perm[..., None].expand(-1, -1, -1, dh))
    v = torch.randint(-8, 9, (B, H, N, dh), generator=gen).float()
    dout = torch.randint(-8, 9, (B, N, H * dh), generator=gen).float()
    return join_qkv(q, k, v), dout, perm, r


def routing_expected(qkv, dout, perm, H, dh=64):
    """The exact results: out[i] = v[perm[i]], dv[perm[i]] = dout[i], dq = dk = 0, the column sums of those, the lse."""
    B, N, _ = qkv.shape
    _, _, v = split_qkv(qkv, H, dh)
    idx = perm[..., None].expand(-1, -1, -1, dh)
    out = unheads(torch.gather(v, 2, idx))
    dv = torch.zeros(B, H, N, dh).scatter_(2, idx, heads(dout, H, dh))
    zero = torch.zeros_like(dv)
    dqkv = join_qkv(zero, zero, dv)
    return out, dqkv, dqkv.sum(1), ROUTING_MULT[dh] ** 2 * dh * float(torch.tensor(dh ** -0.5, dtype=torch.float32))


def routing_gap(r, dh):
    """Smallest distance, in score units, between a query's own key and any other key."""
    N = r.shape[2]
    dots = r @ r.transpose(-2, -1)
    dots.diagonal(dim1=-2, dim2=-1).fill_(-dh)
    worst = float(dots.max()) if N > 1 else -float(dh)
    return worst, ROUTING_MULT[dh] ** 2 * dh ** -0.5 * (dh - worst)


@pytest.mark.parametrize("dh,N", ROUTING_CASES)
def test_routing_builder_gives_an_exact_permutation_softmax(dh, N):
    B, H = 2, 3
    qkv, dout, perm, r = routing_inputs(B, N, H, dh)
    worst, gap = routing_gap(r, dh)
    if dh == 64:
        assert worst <= 48
    assert gap >= ROUTING_MIN_GAP[dh], (worst, gap)
    for x in (qkv, dout):                                   # exact in both 16-bit operand types
        assert torch.equal(x.to(torch.bfloat16).float(), x) and torch.equal(x.half().float(), x)
    q, k, v = split_qkv(qkv, H, dh)
    s = (q @ k.transpose(-2, -1)) * torch.tensor(dh ** -0.5, dtype=torch.float32)
    want = torch.zeros(B, H, N, N).scatter_(3, perm[..., None], 1.0)
    assert torch.equal(s.softmax(-1), want)                 # fp32 softmax: exactly the permutation matrix
    out, dqkv, colsum, lse = routing_expected(qkv, dout, perm, H, dh)
    assert torch.equal(torch.logsumexp(s, -1), torch.full((B, H, N), lse))
    if dh == 64:
        assert lse == 512.0
    assert torch.equal(unheads(want @ v), out)
    # fp64 autograd agrees with the closed form, and every partial sum is an integer below 2^24
    ref = qkv.double().requires_grad_(True)
    q64, k64, v64 = split_qkv(ref, H, dh)
    o64 = unheads(((q64 @ k64.transpose(-2, -1)) * dh ** -0.5).softmax(-1) @ v64)
    o64.backward(dout.double())
    # (fp64 keeps exp(-128) = 3e-56: invisible next to 1, visible next to an exact 0)
    assert float((o64.detach() - out).abs().max()) < 1e-40 and float((ref.grad - dqkv).abs().max()) < 1e-40
    assert float((heads(dout, H, dh).abs() * heads(out, H, dh).abs()).sum(-1).max()) < 2 ** 24


# ---------------------------------------------------------------- random inputs of the fp64 comparison
DISTS = ("plain", "peaked", "offset")


def random_inputs(family, dist, B, N, H, seed=1, dh=64):
    """qkv [B, N, 3*H*dh] ROUNDED to the family's operand type (held in fp32) and dout (bf16-rounded for bf16).  plain: the inputs
    of tests/test_hip_ops.py; peaked: q and k times 4 (a few keys dominate each row); offset: 5.0 added to every feature of every
    key and query (|c|^2 * scale = 200: every score sits near +200 and only the max subtraction keeps exp finite; at another width
    the constant that keeps that 200: c = sqrt(200 / sqrt(dh)))."""
    std = 1.2 if family == "half" else 1.5
    x = (torch.randn(B, N, 3, H, dh, generator=g(seed)) * std)
    if dist == "peaked":
        x[:, :, :2] *= 4.0
    elif dist == "offset":
        x[:, :, :2] += math.sqrt(200.0 / math.sqrt(dh))       # 5.0 at 64
    dout = torch.randn(B, N, H * dh, generator=g(seed + 1))
    x = x.view(B, N, 3 * H * dh).to(OPERAND[family]).float()
    if family == "bf16":
        dout = dout.to(torch.bfloat16).float()
    return x, dout


def exact_fp64(qkv, dout, H, dh=64):
    """fp64 autograd on the given (already rounded) inputs -> out, lse, dqkv"""
    ref = qkv.double().requires_grad_(True)
    q, k, v = split_qkv(ref, H, dh)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    out = unheads(s.softmax(-1) @ v)
    out.backward(dout.double())
    return out.detach(), torch.logsumexp(s.detach(), -1), ref.grad


def half_grad_scale(dout, H):
    """The power of two of mv_attention_bwd_prep_f16 per (image, head): the largest |dout| of the slice goes to [2^7, 2^8)."""
    amax = heads(dout, H).abs().amax((2, 3))
    e = torch.frexp(amax.float())[1]
    return torch.where(amax > 0, torch.ldexp(torch.ones_like(amax, dtype=torch.float32), 8 - e), torch.ones_like(amax)).double()


LOG2E32 = float(torch.tensor(1.4426950408889634, dtype=torch.float32))
LN2_32 = float(torch.tensor(0.6931471805599453, dtype=torch.float32))


def emulate(family, qkv, dout, H, rounded=True, dh=64, blockwise=False):
    """The kernels' rounding model in plain torch -> out, lse, dqkv (fp64 tensors holding the rounded values).

    All three families work in log2 units: the raw fp32 score sum times sl2 = fp32(scale * log2(e)), rounded; the forward takes
    exp2(s2 - max), divides by the unrounded row sum and saves lse = fp32(fp32(max + log2(sum)) * ln(2)); the backward rebuilds
    P = exp2(fma(score, sl2, -fp32(lse * log2(e)))) -- four fp32 roundings at the size of the score, which is what limits the fp32
    kernels when scores reach +-200.  delta, dP and dS are fp32.
    Every product is accumulated in fp32 instruction by instruction (mm below); delta = rowsum(dO * O) is an fp32 sum.
    bf16 / half (csrc/attention.hip): P is rounded to the operand type before P.V and P^T.dO (pack8t of
    csrc/attention_common.h), dS before dS.K and dS^T.Q.  bf16: O and dqkv are rounded to bf16, delta = rowsum(dO * O) reads that rounded O, dS carries
    the softmax scale.  half: O stays fp32; dO is multiplied by a power of two per (image, head) and rounded to half, delta uses the
    rounded dO, dS is formed without the softmax scale (applied to the fp32 dQ / dK), the power of two is divided out at the end.
    fp32 (csrc/attention_f32.hip): nothing is rounded below fp32.
    rounded=False: no rounding at all -- the model must then reproduce fp64 autograd.
    dh: the head width (bf16 only beyond 64); the softmax scale is fp32(dh^-0.5), as the entry points receive it.
    blockwise=True: the key-tiled kernels (attn_fwd_kernel of csrc/attention_tiled.hip, attn_fwd_long_f32_kernel of
    csrc/attention_f32.hip).  Their backward has the whole-head kernels' roundings (P rebuilt from the saved lse, 32 consecutive
    rows per 16x16x32 instruction, fp32: rows 16 T + 4 g + r) except delta of the fp32 family, which attn_delta_long_f32_kernel
    sums as the half prep kernel does: four features per thread, a 16-thread tree.  Their forward is an online softmax over
    64-key blocks: per block the maximum mb of the block's scores, mn = max(m, mb), alpha = exp2(m - mn) (0 on the first block),
    P = exp2(s2 - mn) against the RUNNING maximum, l_g = fp32(l_g * alpha) + the block's P in key order for each of the four lane
    groups g (key j of the block sits in group (j >> 2) & 3), O = fp32(O * alpha), then O += P.V of the block with P rounded to
    the operand type; at the end l = (l_0 + l_1) + (l_2 + l_3), O = fp32(O * fp32(1 / l)) (a rounded reciprocal, not a division)
    and lse = fp32(fp32(m + log2(l)) * ln(2))."""
    if not rounded:
        op = f32 = lambda x: x                                                   # noqa: E731
    else:
        op = lambda x: x.to(OPERAND[family]).double()                            # noqa: E731
        f32 = lambda x: x.float().double()                                       # noqa: E731

    def mm(a, b, over="features", acc=None):
        """a @ b (+ acc) as the matrix instructions accumulate it.  bf16 / half: 16x16x32 -- the 32 products of an instruction (exact in
        fp32) are summed before the one rounding into the accumulator, 32 consecutive indices of the contraction per instruction.
        fp32: 16x16x4 with the four lane groups as its contraction, one fp32 rounding per product, in the kernel's order --
        features 16 c + 4 g + kk for (c, kk, g) (load_global / load_rows of attention_f32.hip), keys or queries 16 T + 4 g + r for
        (T, r, g).  Where dP - delta cancels (one key owns the row) these roundings are the whole error of dS: a model that sums
        in another grouping has errors of the same size but not the same errors, and a slice of few rows shows the difference
        (measured: the half kernel at N = 16 sits at 2.78x a sequential sum's error and at 1.01x this one's)."""
        if not rounded:
            return a @ b if acc is None else acc + a @ b
        K = a.shape[-1]
        if family != "fp32":
            groups = [list(range(i, min(i + 32, K))) for i in range(0, K, 32)]
        elif over == "features":
            groups = [[16 * c + 4 * gg + kk] for c in range(4) for kk in range(4) for gg in range(4)]
        else:
            groups = [[i] for t in range((K + 15) // 16) for r in range(4) for i in (16 * t + 4 * gg + r for gg in range(4)) if i < K]
        if acc is None:
            acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=torch.float64)
        for idx in groups:
            if idx:
                acc = f32(acc + a[..., idx] @ b[..., idx, :])
        return acc

    q, k, v = split_qkv(qkv.double(), H, dh)
    do = heads(dout.double(), H, dh)
    scale = float(torch.tensor(dh ** -0.5, dtype=torch.float32)) if rounded else dh ** -0.5      # (64: 0.125 either way)
    sl2 = float(f32(torch.tensor(scale * LOG2E32, dtype=torch.float64))) if rounded else scale * math.log2(math.e)
    log2e, ln2 = (LOG2E32, LN2_32) if rounded else (math.log2(math.e), math.log(2.0))
    raw = mm(q, k.transpose(-2, -1))
    s2 = f32(raw * sl2)
    if blockwise:
        N = s2.shape[-1]
        m = torch.full(s2.shape[:-1] + (1,), -math.inf, dtype=torch.float64)
        lg = torch.zeros(s2.shape[:-1] + (4,), dtype=torch.float64)
        o = torch.zeros_like(q)
        for k0 in range(0, N, 64):
            blk = slice(k0, min(k0 + 64, N))
            mn = torch.maximum(m, s2[..., blk].amax(-1, keepdim=True))
            alpha = f32(torch.exp2(f32(m - mn)))
            m = mn
            p = f32(torch.exp2(f32(s2[..., blk] - mn)))
            lg = f32(lg * alpha)
            for kt in range(0, p.shape[-1], 16):               # a lane adds its keys 16 kt + 4 g + r in the order (kt, r)
                for r in range(4):
                    cols = [kt + 4 * gg + r for gg in range(4)]
                    live = [c for c in cols if c < p.shape[-1]]
                    lg[..., :len(live)] = f32(lg[..., :len(live)] + p[..., live])
            o = mm(op(p), v[..., blk, :], "rows", acc=f32(o * alpha))
        l = f32(f32(lg[..., 0:1] + lg[..., 1:2]) + f32(lg[..., 2:3] + lg[..., 3:4]))
        out = f32(o * f32(1.0 / l))
    else:
        m = s2.amax(-1, keepdim=True)
        p = f32(torch.exp2(f32(s2 - m)))
        l = p.sum(-1, keepdim=True)
        out = f32(mm(op(p), v, "rows") / l)
    lse = f32(f32(m + torch.log2(l)) * ln2)
    if family == "bf16":
        out = op(out)
    gs = None
    if family == "half" and rounded:
        gs = half_grad_scale(dout, H)[:, :, None, None]
        do = op(do * gs)
    # (fp32 products and sums: where one key dominates, dP - delta cancels and this sum's own rounding is what is left)
    x = do * out                                           # (products of two fp32 values: exact here)
    if not rounded:
        delta = x.sum(-1, keepdim=True)
    elif family == "fp32" and not blockwise:               # attn_bwd_f32_kernel: an fma chain per lane group, then two shuffles
        part = []
        for gg in range(4):
            acc = torch.zeros_like(x[..., 0])
            for c in range(4):
                for e in range(4):
                    acc = f32(acc + x[..., 16 * c + 4 * gg + e])
            part.append(acc)
        delta = f32(f32(part[0] + part[1]) + f32(part[2] + part[3])).unsqueeze(-1)
    elif family in ("half", "fp32"):                       # attn_bwd_prep_f16_kernel: four features per thread, a 16-thread tree
        part = [f32(f32(f32(f32(x[..., 4 * t]) + x[..., 4 * t + 1]) + x[..., 4 * t + 2]) + x[..., 4 * t + 3]) for t in range(16)]
        while len(part) > 1:
            part = [f32(part[i] + part[i + 1]) for i in range(0, len(part), 2)]
        delta = part[0].unsqueeze(-1)
    else:
        delta = x.float().sum(-1, keepdim=True).double()
    p = f32(torch.exp2(f32(raw * sl2 - f32(lse * log2e))))
    dp = mm(do, v.transpose(-2, -1))
    if family == "half":
        ds = op(f32(p * f32(dp - delta)))
        dq, dk = mm(ds, k, "rows") * scale, mm(ds.transpose(-2, -1), q, "rows") * scale
    else:
        ds = op(f32(f32(p * f32(dp - delta)) * scale))
        dq, dk = mm(ds, k, "rows"), mm(ds.transpose(-2, -1), q, "rows")
    dv = mm(op(p).transpose(-2, -1), do, "rows")
    if gs is not None:
        dq, dk, dv = dq / gs, dk / gs, dv / gs
    dqkv = join_qkv(dq, dk, dv)
    dqkv = op(dqkv) if family == "bf16" else f32(dqkv)
    return unheads(out), lse.squeeze(-1), dqkv


def zero_gradient_bound(qkv, dout, H, dh=64):
    """N = 1: softmax is the constant 1, dq = dk = 0 exactly, and relative errors mean nothing.  What a kernel may leave is the
    difference of two fp32 sums of the same 64 products dO_d v_d taken in different orders (dP and delta), times |k| or |q| and the
    scale: |dq|, |dk| <= dh * 2^-23 * sum_d |dO_d v_d| * scale * max |q or k| per (image, head)."""
    q, k, v = split_qkv(qkv.double(), H, dh)
    s = (heads(dout.double(), H, dh).abs() * v.abs()).sum(-1).amax(-1)                   # [B, H]
    return dh * 2.0 ** -23 * s * dh ** -0.5 * torch.maximum(q.abs().amax((2, 3)), k.abs().amax((2, 3)))


def slice_err(got, want, H, dh=64):
    """L2 relative error of dq, dk, dv per (image, head): [3, B, H]"""
    a, b = torch.stack(tuple(split_qkv(got.double().cpu(), H, dh))), torch.stack(tuple(split_qkv(want.double(), H, dh)))
    return (a - b).flatten(3).norm(dim=3) / b.flatten(3).norm(dim=3).clamp_min(1e-300)


def forward_bound(family, qkv, H, dh=64, blocks=0):
    """|out - want| <= ((2 u_P + u_out) + dh * 2^-23 * max_k sum_d |q_d k_d| * scale) * max_k |v_k| per (image, query, head, feature):
    P rounded once (and, in the row sum, not at all: twice u_P covers a truncating pack), the output rounded once, the fp32 score sum.

    blocks = ceil(N / 64) > 0: the online form of the key-tiled kernels.  P is rounded against the running maximum instead of the
    final one, but a rounding to the operand type is relative, so its term is unchanged: the later factors alpha multiply the
    rounded value.  The error of alpha itself multiplies O and l alike and leaves O / l.  What the online form adds, relative
    to the running |O| <= l * max |v| (every P is positive, so running sums never exceed final ones):
        per block   2^-24 * (1 [O * alpha] + 2 [the block's two accumulating P.V instructions] + 1 [l * alpha] + 16 [the lane's 16
                    additions to l])                                                                          = 20 * 2^-24
        at the end  2^-24 * (2 [the two shuffle additions of l] + 1 [1 / l rounded] + 1 [O * (1 / l) rounded])  =  4 * 2^-24
    so the bound grows by (20 * blocks + 4) * 2^-24 * max |v|."""
    q, k, v = split_qkv(qkv.double(), H, dh)
    ssum = (q.abs() @ k.abs().transpose(-2, -1)).amax(-1, keepdim=True) * dh ** -0.5     # [B, H, N, 1]
    vmax = v.abs().amax(2, keepdim=True)                                                 # [B, H, 1, dh]
    online = (20 * blocks + 4) * 2.0 ** -24 if blocks else 0.0
    return unheads((2 * U_P[family] + U_OUT[family] + dh * 2.0 ** -23 * ssum + online) * vmax)


def lse_bound(qkv, H, lse, dh=64, blocks=0):
    """the fp32 score sum, then four fp32 roundings of a value of the size of the lse.
    blocks = ceil(N / 64) > 0: the online form.  lse = (m + log2(l)) ln 2 with a running sum l.  A relative error of l is that
    absolute error of ln(l); what the online form adds to it, in units of 2^-24:
        per block   1 [l * alpha rounded] + 1 [exp2 of alpha] + 1 [the rounding of m - mn, an error of the exponent of
                    2^-24 |m - mn| ln 2 weighted by alpha = 2^-|m - mn|: at most 0.53] + 16 [the lane's additions]     = 19
        at the end  2 [the two shuffle additions]
    (here alpha's own error does not cancel: there is no quotient)."""
    q, k, _ = split_qkv(qkv.double(), H, dh)
    ssum = (q.abs() @ k.abs().transpose(-2, -1)).amax(-1) * dh ** -0.5
    online = (19 * blocks + 2) * 2.0 ** -24 if blocks else 0.0
    return dh * 2.0 ** -23 * ssum + 4 * 2.0 ** -24 * lse.abs() + online


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dist", DISTS)
def test_emulation_is_consistent_with_fp64(family, dist):
    B, N, H = 2, 197, 2
    qkv, dout = random_inputs(family, dist, B, N, H, seed=3)
    assert torch.equal(qkv.to(OPERAND[family]).float(), qkv)
    q, k, _ = split_qkv(qkv.double(), H)
    s = (q @ k.transpose(-2, -1)) * SCALE
    if dist == "peaked":
        assert float(s.abs().max()) > (60 if family == "half" else 100) and float(s.softmax(-1).amax(-1).median()) > 0.5
    if dist == "offset":
        assert 150 < float(s.mean()) < 260 and float(s.min()) > 88.8          # exp(s) alone overflows fp32 everywhere
    want = exact_fp64(qkv, dout, H)
    for a, b in zip(emulate(family, qkv, dout, H, rounded=False), want):         # the formulas: fp64 autograd to rounding noise
        assert relmax(a, b) < 1e-11
    out, lse, dqkv = emulate(family, qkv, dout, H)
    u = {"bf16": 2.0 ** -9, "half": 2.0 ** -12, "fp32": 2.0 ** -24}[family]
    err = slice_err(dqkv, want[2], H)
    assert float(err.max()) < 1.0 and float(err.min()) > u / 64, (float(err.min()), float(err.max()))   # rounds, and not wildly
    if family != "fp32":
        assert bool(((out - want[0]).abs() <= forward_bound(family, qkv, H)).all())
        assert float(err.min()) > 2.0 ** -24 * 16
    assert bool(((lse - want[1]).abs() <= lse_bound(qkv, H, want[1])).all())
    if dist == "plain":
        assert relmax(out, want[0]) < CEIL[family][0] and relmax(dqkv, want[2]) < CEIL[family][1]
    if family == "half":                                                         # the power of two: the largest |dout| -> [128, 256)
        gs = half_grad_scale(dout * 3.0e-7, H)
        top = heads(dout * 3.0e-7, H).abs().amax((2, 3)).double() * gs
        assert bool(((top >= 128) & (top < 256)).all()) and bool((torch.log2(gs) == torch.log2(gs).round()).all())


# ================================================================== the raw entry points, on any allocation
@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    _ops.lib()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return _ops


def L():
    from myrtle_vision.hip.lib import lib
    return lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


@contextmanager
def forced(fwd=0, bwd=0):
    """mv_attention_fwd_force / _bwd_force for the calls inside; always back to automatic."""
    try:
        assert L().mv_attention_fwd_force(fwd) == MV_OK and L().mv_attention_bwd_force(bwd) == MV_OK
        yield
    finally:
        L().mv_attention_fwd_force(0)
        L().mv_attention_bwd_force(0)


SENTINEL = 0xA5


def poison(t):
    if t.is_floating_point():
        t.fill_(float("nan"))
    else:
        t.fill_(0x55)
    return t


class Tight:
    """plain tensors"""
    def inp(self, data, dtype=None):
        return data.to(device="cuda", dtype=dtype or data.dtype).contiguous().clone()

    def out(self, shape, dtype):
        return poison(torch.empty(shape, dtype=dtype, device="cuda"))

    def check(self):
        torch.cuda.synchronize()


class Guarded:
    """Every tensor a 16-byte-aligned view in the middle of a larger allocation: at least 32 rows' worth of elements on each side,
    NaN next to inputs, a sentinel byte pattern round outputs, the output body prefilled with NaN.  check(): no guard byte changed,
    no input changed, every output element finite."""
    def __init__(self):
        self.inputs, self.outputs = [], []

    def _carve(self, shape, dtype):
        n, es = math.prod(shape), torch.empty((), dtype=dtype).element_size()
        guard = (32 * max(shape[-1], 64) + 15) // 16 * 16
        raw = torch.empty((n + 2 * guard) * es, dtype=torch.uint8, device="cuda")
        body = raw[guard * es:(guard + n) * es].view(dtype).view(shape)
        assert body.data_ptr() % 16 == 0 and body.data_ptr() == raw.data_ptr() + guard * es
        return raw, body, guard * es, n * es

    def inp(self, data, dtype=None):
        data = data.to(device="cuda", dtype=dtype or data.dtype)
        raw, body, _, _ = self._carve(tuple(data.shape), data.dtype)
        raw.view(data.dtype).fill_(float("nan"))
        body.copy_(data)
        self.inputs.append((raw, raw.clone()))
        return body

    def out(self, shape, dtype):
        raw, body, gb, nb = self._carve(tuple(shape), dtype)
        raw.fill_(SENTINEL)
        poison(body)
        self.outputs.append((raw, body, gb, nb))
        return body

    def check(self):
        torch.cuda.synchronize()
        for raw, before in self.inputs:
            assert torch.equal(raw, before), "an input or its guard was written"
        for raw, body, gb, nb in self.outputs:
            assert bool((raw[:gb] == SENTINEL).all()) and bool((raw[gb + nb:] == SENTINEL).all()), "a guard byte changed"
            if body.is_floating_point():
                assert bool(torch.isfinite(body.float()).all()), "an output element was left unwritten or is not finite"


def run_fwd(A, family, qkv, B, N, H, variant=0, kind="lse", scale=SCALE):
    """-> dict of outputs.  bf16: variant = mv_attention_fwd_force value.  fp32: kind "plain" | "lse" | "q8"."""
    C = H * 64
    q = A.inp(qkv, OPERAND[family])
    r = {}
    if family == "bf16":
        r["out"], r["lse"] = A.out((B, N, C), torch.bfloat16), A.out((B, H, N), torch.float32)
        with forced(fwd=variant):
            rc = L().mv_attention_fwd(ptr(q), ptr(r["out"]), ptr(r["lse"]), B, N, H, scale, stream())
    elif family == "half":
        r["out"], r["lse"] = A.out((B, N, C), torch.float32), A.out((B, H, N), torch.float32)
        rc = L().mv_attention_fwd_f16(ptr(q), ptr(r["out"]), ptr(r["lse"]), B, N, H, scale, stream())
    elif kind == "plain":
        r["out"] = A.out((B, N, C), torch.float32)
        rc = L().mv_attention_fwd_f32(ptr(q), ptr(r["out"]), B, N, H, scale, stream())
    elif kind == "lse":
        r["out"], r["lse"] = A.out((B, N, C), torch.float32), A.out((B, H, N), torch.float32)
        rc = L().mv_attention_fwd_f32_lse(ptr(q), ptr(r["out"]), ptr(r["lse"]), B, N, H, scale, stream())
    else:
        r["codes"] = A.out((B, N, C), torch.int8)
        rc = L().mv_attention_fwd_f32_q8(ptr(q), ptr(r["codes"]), B, N, H, scale, Q8_SCALE, Q8_ZERO, stream())
    assert rc == MV_OK, (family, kind, variant, N, rc)
    A.check()
    return r


Q8_SCALE, Q8_ZERO = 0.125, 128          # integers in [-8, 8] sit on the grid: code = 8 * v


def run_bwd(A, family, qkv, fw, dout, B, N, H, variant=0, scale=SCALE):
    """fw: the forward's out / lse.  bf16: variant = mv_attention_bwd_force value -> dqkv, colsum.  half: variant = nseg (0, 3, 6)
    -> dqkv (fp32, or the bf16 pieces), colsum, and the prep kernel's dout16 / delta / gscale.  fp32 -> dqkv."""
    C = H * 64
    q = A.inp(qkv, OPERAND[family])
    out, lse = A.inp(fw["out"]), A.inp(fw["lse"])
    r = {}
    if family == "bf16":
        d = A.inp(dout, torch.bfloat16)
        r["dqkv"], r["colsum"] = A.out((B, N, 3 * C), torch.bfloat16), A.out((B, 3 * C), torch.float32)
        with forced(bwd=variant):
            rc = L().mv_attention_bwd(ptr(q), ptr(out), ptr(d), ptr(lse), ptr(r["dqkv"]), ptr(r["colsum"]), B, N, H, scale, stream())
    elif family == "half":
        d = A.inp(dout, torch.float32)
        r["dout16"], r["delta"] = A.out((B, N, C), torch.float16), A.out((B, H, N), torch.float32)
        r["gscale"] = A.out((B * H,), torch.float32)
        rc = L().mv_attention_bwd_prep_f16(ptr(d), ptr(out), ptr(r["dout16"]), ptr(r["delta"]), ptr(r["gscale"]), B, N, H, stream())
        assert rc == MV_OK, (N, rc)
        A.check()
        d16, dl, gs = A.inp(r["dout16"]), A.inp(r["delta"]), A.inp(r["gscale"])
        r["colsum"] = A.out((B, 3 * C), torch.float32)
        r["dqkv"] = A.out((B * N, variant * 3 * C), torch.bfloat16) if variant else A.out((B, N, 3 * C), torch.float32)
        rc = L().mv_attention_bwd_f16(ptr(q), ptr(d16), ptr(dl), ptr(lse), ptr(gs), ptr(r["dqkv"]), variant, ptr(r["colsum"]),
                                      B, N, H, scale, stream())
    else:
        d = A.inp(dout, torch.float32)
        r["dqkv"] = A.out((B, N, 3 * C), torch.float32)
        rc = L().mv_attention_bwd_f32(ptr(q), ptr(out), ptr(d), ptr(lse), ptr(r["dqkv"]), B, N, H, scale, stream())
    assert rc == MV_OK, (family, variant, N, rc)
    A.check()
    return r


def fwd_kinds(family):
    """(variant, kind) of every forward kernel of the family"""
    return [(v, "lse") for v in FWD_VARIANTS] if family == "bf16" else [(0, "lse")] if family == "half" else \
        [(0, "plain"), (0, "lse"), (0, "q8")]


def bwd_kinds(family, N):
    return bwd_variants(N) if family == "bf16" else [0, 3, 6] if family == "half" else [0]


def split_of(ops, dqkv, nseg):
    """the bf16 pieces of an fp32 dqkv [B, N, 3C], as the split-operand products read them"""
    rows, cols = dqkv.shape[0] * dqkv.shape[1], dqkv.shape[2]
    with ops.segments(nseg):
        return ops.split_ex(dqkv.contiguous().view(rows, cols), rows, cols)


# ================================================================== 1. routing
def assert_routed_forward(family, r, want_out, want_lse, kind, tag):
    if "lse" in r:
        assert float((r["lse"].double().cpu() - want_lse).abs().max()) <= 4 * 2.0 ** -24 * want_lse, tag
    if kind == "q8":
        assert torch.equal(r["codes"].cpu(), (want_out * 8).to(torch.int8)), tag
    elif family == "fp32":
        assert bool(((r["out"].cpu() - want_out).abs() <= 2 * 2.0 ** -14 * want_out.abs()).all()), tag
    else:
        assert torch.equal(r["out"].float().cpu(), want_out), tag


def assert_routed_backward(ops, family, variant, r, want_dqkv, want_colsum, H, tag, dh=64):
    if family == "half" and variant:
        assert torch.equal(r["dqkv"], split_of(ops, want_dqkv.cuda(), variant)), tag
    else:
        dq, dk, dv = split_qkv(r["dqkv"].float().cpu(), H, dh)
        assert bool((dq == 0).all()) and bool((dk == 0).all()), tag
        want_dv = split_qkv(want_dqkv, H, dh)[2]
        if family == "fp32":
            assert bool(((dv - want_dv).abs() <= 2 * 2.0 ** -14 * want_dv.abs()).all()), tag
        else:
            assert torch.equal(dv, want_dv), tag
    if "colsum" in r:
        C = H * dh
        cs = r["colsum"].cpu()
        assert bool((cs[:, :2 * C] == 0).all()) and torch.equal(cs[:, 2 * C:], want_colsum[:, 2 * C:]), tag


@gpu
@pytest.mark.parametrize("family,N", family_lengths(EDGES))
def test_routing_is_exact_in_every_kernel(ops, family, N):
    """Softmax = a permutation matrix: out[i] = v[perm[i]], dv[perm[i]] = dout[i], dq = dk = 0, bit for bit, in every kernel that
    takes the length (fp32: P is not rounded, so out / dv carry the 2 ulp of the lse at 512)."""
    B, H = 2, 3
    qkv, dout, perm, _ = routing_inputs(B, N, H)
    want_out, want_dqkv, want_colsum, want_lse = routing_expected(qkv, dout, perm, H)
    A = Tight()
    fw = None
    for variant, kind in fwd_kinds(family):
        r = run_fwd(A, family, qkv, B, N, H, variant, kind)
        assert_routed_forward(family, r, want_out, want_lse, kind, (variant, kind))
        if "lse" in r and fw is None:
            fw = r
    for variant in bwd_kinds(family, N):
        r = run_bwd(A, family, qkv, fw, dout, B, N, H, variant)
        assert_routed_backward(ops, family, variant, r, want_dqkv, want_colsum, H, variant)


@gpu
@pytest.mark.parametrize("name,N", [("long", 577), ("long", 1025), ("long_f16", 577), ("long_f32", 577)])
def test_routing_is_exact_in_the_key_tiled_kernels(ops, name, N):
    B, H = 2, 3
    qkv, dout, perm, _ = routing_inputs(B, N, H)
    want_out, want_dqkv, want_colsum, want_lse = routing_expected(qkv, dout, perm, H)
    if name == "long":
        q = qkv.to(torch.bfloat16).cuda()
        out, lse = ops.attention_fwd_long(q, B, N, H, SCALE)
        colsum = poison(torch.empty(B, 3 * H * 64, device="cuda"))
        dqkv = ops.attention_bwd_long(q, out, dout.to(torch.bfloat16).cuda(), lse, B, N, H, SCALE, colsum=colsum)
        family, r = "bf16", {"dqkv": dqkv, "colsum": colsum}
    elif name == "long_f16":
        q = qkv.half().cuda()
        out, lse = ops.attention_fwd_long_f16(q, B, N, H, SCALE)
        colsum = poison(torch.empty(B, 3 * H * 64, device="cuda"))
        dqkv = ops.attention_bwd_long_f16(q, out, dout.cuda(), lse, B, N, H, SCALE, colsum=colsum)
        family, r = "half", {"dqkv": dqkv, "colsum": colsum}
        for nseg in (3, 6):
            with ops.segments(nseg):
                pieces = ops.attention_bwd_long_f16(q, out, dout.cuda(), lse, B, N, H, SCALE, split=True)
            assert torch.equal(pieces, split_of(ops, want_dqkv.cuda(), nseg)), nseg
    else:
        q = qkv.cuda()
        out, lse = ops.attention_fwd_long_f32(q, B, N, H, SCALE)
        assert same_bits(out, ops.attention_fwd_long_f32(q, B, N, H, SCALE, lse=False))
        codes = ops.attention_fwd_long_f32_q8(q, B, N, H, SCALE, Q8_SCALE, Q8_ZERO)
        assert torch.equal(codes.cpu(), (want_out * 8).to(torch.int8))
        family, r = "fp32", {"dqkv": ops.attention_bwd_long_f32(q, out, dout.cuda(), lse, B, N, H, SCALE)}
    assert_routed_forward(family, {"out": out, "lse": lse}, want_out, want_lse, "lse", name)
    assert_routed_backward(ops, family, 0, r, want_dqkv, want_colsum, H, name)


@gpu
@pytest.mark.parametrize("dh", [32, 128])
@pytest.mark.parametrize("N", [197, 577])
def test_routing_is_exact_in_the_other_head_widths(ops, dh, N):
    B, H = 2, 3
    scale = float(torch.tensor(dh ** -0.5, dtype=torch.float32))
    qkv, dout, perm, _ = routing_inputs(B, N, H, dh)
    want_out, want_dqkv, want_colsum, want_lse = routing_expected(qkv, dout, perm, H, dh)
    q = qkv.to(torch.bfloat16).cuda()
    out, lse = ops.attention_fwd_dh(q, B, N, H, dh, scale)
    assert_routed_forward("bf16", {"out": out, "lse": lse}, want_out, want_lse, "lse", dh)
    colsum = poison(torch.empty(B, 3 * H * dh, device="cuda"))
    dqkv = ops.attention_bwd_dh(q, out, dout.to(torch.bfloat16).cuda(), lse, B, N, H, dh, scale, colsum=colsum)
    assert_routed_backward(ops, "bf16", 0, {"dqkv": dqkv, "colsum": colsum}, want_dqkv, want_colsum, H, dh, dh=dh)


# ================================================================== 2. every edge, every variant, against fp64
@gpu
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("family,N", family_lengths(EDGES))
def test_every_edge_and_variant_against_fp64(ops, family, N, dist):
    """Every kernel that takes the length, on the inputs of tests/test_hip_ops.py and on two harder score distributions, against
    fp64 on the same rounded inputs.  plain: the whole-tensor ceilings of the older tests, and a second launch gives the same bits.
    All: the derived per-element forward bound (bf16, half) and lse bound.  peaked / offset: each of dq, dk, dv per (image, head)
    within 2x the L2 error of the fp64 emulation of the kernel's roundings on the same inputs (fp32: the forward too).

    The emulation has to accumulate as the kernels do (emulate.mm, delta): where one key owns a row, dP - delta cancels and the
    handful of fp32 roundings inside those sums is the whole error of dS, so a model that sums in another order has errors of the
    same size but not the same errors, and on a slice of few rows that alone was worth a factor of 3."""
    B, H = 2, 3
    qkv, dout = random_inputs(family, dist, B, N, H, seed=N)
    want_out, want_lse, want_dqkv = exact_fp64(qkv, dout, H)
    emu_out, _, emu_dqkv = emulate(family, qkv, dout, H)
    emu_err = slice_err(emu_dqkv, want_dqkv, H)
    ceil_f, ceil_b, ceil_lse = CEIL[family]
    A = Tight()
    fw = None
    for variant, kind in fwd_kinds(family):
        r = run_fwd(A, family, qkv, B, N, H, variant, kind)
        tag = (variant, kind)
        if dist == "plain":
            r2 = run_fwd(A, family, qkv, B, N, H, variant, kind)
            assert all(same_bits(r[key], r2[key]) for key in r), tag
        if kind == "q8":
            continue                                       # (codes: the routing and guard tests; tests/test_int8_model.py)
        out = r["out"].double().cpu()
        e = relmax(out, want_out)
        print(f"fwd {family} N={N} {dist} {tag}: max-norm {e:.3e}  emulation {relmax(emu_out, want_out):.3e}")
        if dist == "plain":
            assert e < ceil_f, tag
        if family != "fp32":
            excess = ((out - want_out).abs() / forward_bound(family, qkv, H)).max()
            print(f"    per-element error / bound: {float(excess):.3f}")
            assert float(excess) <= 1.0, tag
        elif dist != "plain":
            got_e, emu_e = rel_l2(out, want_out), rel_l2(emu_out, want_out)
            print(f"    L2 {got_e:.3e}  emulation {emu_e:.3e}")
            assert got_e <= 2 * emu_e, tag
        if "lse" in r:
            d = (r["lse"].double().cpu() - want_lse).abs()
            assert bool((d <= lse_bound(qkv, H, want_lse)).all()), tag
            if dist == "plain":
                assert float(d.max()) < ceil_lse, tag
            fw = fw or r
    plain, parts = None, "qkv"
    for variant in bwd_kinds(family, N):
        r = run_bwd(A, family, qkv, fw, dout, B, N, H, variant)
        if dist == "plain":
            r2 = run_bwd(A, family, qkv, fw, dout, B, N, H, variant)
            assert all(same_bits(r[key], r2[key]) for key in r), variant
        if family == "half" and variant:                   # the pieces of exactly the plain form's fp32 values, and its column sums
            assert torch.equal(r["dqkv"], split_of(ops, plain["dqkv"], variant)), variant
            assert relmax(r["colsum"], plain["dqkv"].double().sum(1)) < 1e-5, variant
            continue
        plain = r
        got = r["dqkv"].double().cpu()
        err = slice_err(got, want_dqkv, H)
        if N == 1:                                         # dq = dk = 0 exactly: an absolute bound, and only dv is relative
            zb = zero_gradient_bound(qkv, dout, H)[:, :, None, None]
            assert all(bool((split_qkv(got, H)[i].abs() <= zb).all()) for i in (0, 1)), variant
            err, parts = err[2:], "v"
        ratio = (err / emu_err[-len(err):]).amax((1, 2))
        print(f"bwd {family} N={N} {dist} v{variant}: max-norm {relmax(got, want_dqkv):.3e}  worst slice L2 dq/dk/dv "
              f"{[f'{float(x):.3e}' for x in err.amax((1, 2))]}  emulation {[f'{float(x):.3e}' for x in emu_err.amax((1, 2))]}  "
              f"worst ratio {[f'{float(x):.2f}' for x in ratio]}")
        if dist == "plain":
            for i, name in enumerate("qkv"):
                if name in parts:
                    assert relmax(split_qkv(got, H)[i], split_qkv(want_dqkv, H)[i]) < ceil_b, (variant, name)
        elif N == 1:                                       # dv = P dO with one P per slice: no statistics for a factor of 2 to cover.
            # P is 1 up to the four fp32 roundings of its exponent, at the size of the lse; then the output rounding
            # (bf16) or the rounding of dO to half, and P itself rounded to the operand type
            bar = 4 * 2.0 ** -24 * max(1.0, float(want_lse.abs().max())) + {"bf16": 2.0 ** -8, "half": 2.0 ** -11, "fp32": 2.0 ** -23}[family]
            assert float(err.max()) <= bar, (variant, float(err.max()), bar)
        else:
            assert bool((err <= 2 * emu_err).all()), (variant, [float(x) for x in ratio])
        if "colsum" in r:                                  # fp32 sums of the accumulators, before the output rounding
            cs = r["colsum"].double().cpu()
            if dist == "plain":
                assert relmax(cs, want_dqkv.sum(1)) < ceil_b, variant
                assert relmax(cs, got.sum(1)) < (5e-3 if family == "bf16" else 1e-5), variant


# ================================================================== 3. guard zones
@gpu
@pytest.mark.parametrize("family,N", family_lengths(GUARD_N))
def test_nothing_outside_the_tensors_is_read_into_a_result_or_written(ops, family, N):
    """Every input next to NaN, every output between sentinels and prefilled with NaN (Guarded.check), for every kernel that takes
    the length; and the bits of the same call on plain tensors."""
    B, H = 2, 3
    qkv, dout = random_inputs(family, "plain", B, N, H, seed=100 + N)
    tight_fw = None
    for variant, kind in fwd_kinds(family):
        t, gd = run_fwd(Tight(), family, qkv, B, N, H, variant, kind), run_fwd(Guarded(), family, qkv, B, N, H, variant, kind)
        assert all(same_bits(t[key], gd[key]) for key in t), (variant, kind)
        if "lse" in t and tight_fw is None:
            tight_fw = t
    for variant in bwd_kinds(family, N):
        t = run_bwd(Tight(), family, qkv, tight_fw, dout, B, N, H, variant)
        gd = run_bwd(Guarded(), family, qkv, tight_fw, dout, B, N, H, variant)
        assert all(same_bits(t[key], gd[key]) for key in t), variant


# ================================================================== 4. independence, permutation, zero gradient
@gpu
@pytest.mark.parametrize("family,N", family_lengths([197, 257, 320]))
def test_every_image_and_head_is_computed_alone(ops, family, N):
    """One workgroup owns one (image, head) and its arithmetic does not depend on B or H: each slice run as a B = 1, H = 1 problem
    gives the bits of the batched run."""
    B, H = 3, 3
    qkv, dout = random_inputs(family, "plain", B, N, H, seed=200 + N)
    A = Tight()
    fws = [run_fwd(A, family, qkv, B, N, H, 0, kind) for _, kind in fwd_kinds(family) if _ == 0]
    fw = next(r for r in fws if "lse" in r)
    bws = {v: run_bwd(A, family, qkv, fw, dout, B, N, H, v) for v in bwd_kinds(family, N)}
    q, k, v = split_qkv(qkv, H)
    do = heads(dout, H)
    for b in range(B):
        for h in range(H):
            one = join_qkv(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1])
            d1 = unheads(do[b:b + 1, h:h + 1]).contiguous()
            cols = slice(h * 64, (h + 1) * 64)
            fw1 = None
            for r, (_, kind) in zip(fws, [fk for fk in fwd_kinds(family) if fk[0] == 0]):
                r1 = run_fwd(A, family, one, 1, N, 1, 0, kind)
                for key in r1:
                    full = r[key][b, h] if key == "lse" else r[key][b, :, cols]
                    assert same_bits(full.reshape(-1), r1[key].reshape(-1)), (b, h, kind, key)
                if "lse" in r1:
                    fw1 = r1
            for variant, r in bws.items():
                r1 = run_bwd(A, family, one, fw1, d1, 1, N, 1, variant)
                if family == "half" and variant:
                    got = r["dqkv"].view(B, N, variant, 3, H, 64)[b, :, :, :, h]
                    assert same_bits(got.contiguous(), r1["dqkv"].view(N, variant, 3, 64)), (b, h, variant)
                else:
                    got = r["dqkv"].view(B, N, 3, H, 64)[b, :, :, h]
                    assert same_bits(got.contiguous(), r1["dqkv"].view(N, 3, 64)), (b, h, variant)
                if "colsum" in r:
                    assert same_bits(r["colsum"].view(B, 3, H, 64)[b, :, h].contiguous(), r1["colsum"].view(3, 64)), (b, h, variant)
                if "gscale" in r:
                    assert same_bits(r["gscale"][b * H + h:b * H + h + 1], r1["gscale"]) and \
                        same_bits(r["delta"][b, h], r1["delta"][0, 0]), (b, h)


@gpu
@pytest.mark.parametrize("N", [197, 300])
def test_key_permutation(ops, N):
    """As tests/test_attention_long.py::test_long_attention_key_permutation, for the whole-head bf16 kernels: permuting keys and
    values together leaves the output unchanged up to the order of the fp32 sums and the bf16 rounding of P; dK and dV permute."""
    B, H = 2, 2
    qkv, dout = random_inputs("bf16", "plain", B, N, H, seed=13)
    perm = torch.randperm(N, generator=g(14))
    q5 = qkv.view(B, N, 3, H, 64)
    q5p = q5.clone()
    q5p[:, :, 1] = q5[:, perm, 1]
    q5p[:, :, 2] = q5[:, perm, 2]
    qkvp = q5p.view(B, N, 3 * H * 64)
    A = Tight()
    for fv in FWD_VARIANTS:
        a, b = run_fwd(A, "bf16", qkv, B, N, H, fv), run_fwd(A, "bf16", qkvp, B, N, H, fv)
        assert rel_l2(b["out"].float(), a["out"].float()) < 6e-3, fv
        assert float((b["lse"] - a["lse"]).abs().max()) < 1e-4, fv
    for bv in bwd_variants(N):
        d = run_bwd(A, "bf16", qkv, a, dout, B, N, H, bv)["dqkv"].float().cpu().view(B, N, 3, H, 64)
        dp = run_bwd(A, "bf16", qkvp, b, dout, B, N, H, bv)["dqkv"].float().cpu().view(B, N, 3, H, 64)
        assert rel_l2(dp[:, :, 0], d[:, :, 0]) < 2e-2, bv
        for i in (1, 2):
            assert rel_l2(dp[:, :, i], d[:, perm, i]) < 2e-2, (bv, "kv"[i - 1])


@gpu
@pytest.mark.parametrize("family,N", [(f, n) for f in ("bf16", "fp32") for n in (17, 197, 209, 225, 272, 320) if n <= CAP[f]])
def test_zero_gradient_gives_exact_zeros(ops, family, N):
    B, H = 2, 2
    qkv, dout = random_inputs(family, "plain", B, N, H, seed=300 + N)
    A = Tight()
    fw = run_fwd(A, family, qkv, B, N, H)
    for variant in bwd_kinds(family, N):
        r = run_bwd(A, family, qkv, fw, torch.zeros_like(dout), B, N, H, variant)
        assert not r["dqkv"].any(), variant
        assert "colsum" not in r or not r["colsum"].any(), variant


# ================================================================== 5. API edges: nothing is launched
def api_calls(family, B, N, H, off=0):
    """Every entry point of the family on canary-filled buffers big enough for any length: -> [(name, rc)], the buffers.  off: qkv
    pointer offset in elements."""
    C, n = H * 64 if H else 64, max(N, 1) + 1
    es = {"bf16": 2, "half": 2, "fp32": 4}[family]
    buf = {name: torch.full((max(B, 1) * n * 3 * C * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
           for name in ("qkv", "out", "lse", "dout", "dqkv", "colsum", "aux1", "aux2")}
    p = {name: t.data_ptr() for name, t in buf.items()}
    q, s = p["qkv"] + off * es, stream()
    if family == "bf16":
        rcs = [("fwd", L().mv_attention_fwd(q, p["out"], p["lse"], B, N, H, SCALE, s)),
               ("bwd", L().mv_attention_bwd(q, p["out"], p["dout"], p["lse"], p["dqkv"], p["colsum"], B, N, H, SCALE, s))]
    elif family == "half":
        rcs = [("fwd", L().mv_attention_fwd_f16(q, p["out"], p["lse"], B, N, H, SCALE, s)),
               ("bwd", L().mv_attention_bwd_f16(q, p["dout"], p["aux1"], p["lse"], p["aux2"], p["dqkv"], 0, p["colsum"], B, N, H, SCALE, s))]
    else:
        rcs = [("fwd", L().mv_attention_fwd_f32(q, p["out"], B, N, H, SCALE, s)),
               ("fwd_lse", L().mv_attention_fwd_f32_lse(q, p["out"], p["lse"], B, N, H, SCALE, s)),
               ("fwd_q8", L().mv_attention_fwd_f32_q8(q, p["out"], B, N, H, SCALE, Q8_SCALE, Q8_ZERO, s)),
               ("bwd", L().mv_attention_bwd_f32(q, p["out"], p["dout"], p["lse"], p["dqkv"], B, N, H, SCALE, s))]
    torch.cuda.synchronize()
    return rcs, buf


def untouched(buf):
    return all(bool((t == SENTINEL).all()) for t in buf.values())


@gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_api_edges_return_their_codes_and_write_nothing(ops, family):
    too_long = MV_ERR_SHAPE if family == "bf16" else MV_ERR_UNSUPPORTED           # include/myrtle_vision_hip.h; the entry points
    for (B, N, H, off), want in [((0, 197, 3, 0), MV_OK), ((2, 0, 3, 0), MV_ERR_SHAPE), ((2, CAP[family] + 1, 3, 0), too_long),
                                 ((2, 197, 0, 0), MV_ERR_SHAPE), ((2, 197, 3, 1), MV_ERR_ALIGN), ((2, -1, 3, 0), MV_ERR_SHAPE)]:
        rcs, buf = api_calls(family, B, N, H, off)
        assert all(rc == want for _, rc in rcs), ((B, N, H, off), rcs)
        assert untouched(buf), (B, N, H, off)
    if family == "half":                                                          # the prep pass and the split count
        rcs, buf = api_calls(family, 2, 197, 3)
        p = {name: t.data_ptr() for name, t in buf.items()}
        assert L().mv_attention_bwd_f16(p["qkv"], p["dout"], p["aux1"], p["lse"], p["aux2"], p["dqkv"], 4, p["colsum"], 2, 197, 3,
                                        SCALE, stream()) == MV_ERR_UNSUPPORTED
        for (B, N, H), want in [((0, 197, 3), MV_OK), ((2, 0, 3), MV_ERR_SHAPE), ((2, 197, 0), MV_ERR_SHAPE)]:
            buf2 = {name: torch.full((1 << 20,), SENTINEL, dtype=torch.uint8, device="cuda") for name in "abcde"}
            p2 = [t.data_ptr() for t in buf2.values()]
            assert L().mv_attention_bwd_prep_f16(*p2, B, N, H, stream()) == want
            torch.cuda.synchronize()
            assert untouched(buf2)
        assert L().mv_attention_bwd_prep_f16(p["dout"] + 4, p["out"], p["aux1"], p["lse"], p["aux2"], 2, 197, 3, stream()) == MV_ERR_ALIGN
        torch.cuda.synchronize()


@gpu
def test_forcing_an_unknown_variant_is_rejected(ops):
    B, N, H = 1, 197, 2
    qkv, dout = random_inputs("bf16", "plain", B, N, H, seed=5)
    A = Tight()
    fw = run_fwd(A, "bf16", qkv, B, N, H)
    bw = run_bwd(A, "bf16", qkv, fw, dout, B, N, H)
    try:
        for v in (-1, 4, 5, 8, 14):
            assert L().mv_attention_fwd_force(v) == MV_ERR_UNSUPPORTED, v
        for v in (-1, 1, 3, 6, 7, 9, 20):
            assert L().mv_attention_bwd_force(v) == MV_ERR_UNSUPPORTED, v
        # a rejected value changes nothing: still the automatic choice
        fw2 = {k_: t for k_, t in zip(("out", "lse"), ops.attention_fwd(qkv.to(torch.bfloat16).cuda(), B, N, H, SCALE))}
        assert all(same_bits(fw[key], fw2[key]) for key in fw)
        assert same_bits(bw["dqkv"], ops.attention_bwd(qkv.to(torch.bfloat16).cuda(), fw["out"], dout.to(torch.bfloat16).cuda(),
                                                       fw["lse"], B, N, H, SCALE))
    finally:
        L().mv_attention_fwd_force(0)
        L().mv_attention_bwd_force(0)


@gpu
@pytest.mark.parametrize("variant,N", [(2, 225), (3, 209)])
def test_forced_forward_that_cannot_take_the_length_falls_back(ops, variant, N):
    B, H = 2, 3
    qkv, _ = random_inputs("bf16", "plain", B, N, H, seed=7)
    auto, got = run_fwd(Tight(), "bf16", qkv, B, N, H, 0), run_fwd(Tight(), "bf16", qkv, B, N, H, variant)
    assert same_bits(auto["out"], got["out"]) and same_bits(auto["lse"], got["lse"])


@gpu
@pytest.mark.parametrize("variant,N", [(4, 209), (2, 289)])
def test_forced_backward_that_cannot_take_the_length_falls_back(ops, variant, N):
    """(to a kernel that takes the length -- not necessarily the automatic one: the fp64 bars)"""
    B, H = 2, 3
    qkv, dout = random_inputs("bf16", "plain", B, N, H, seed=9)
    _, _, want = exact_fp64(qkv, dout, H)
    fw = run_fwd(Tight(), "bf16", qkv, B, N, H)
    r = run_bwd(Guarded(), "bf16", qkv, fw, dout, B, N, H, variant)
    got = r["dqkv"].double().cpu()
    for i, name in enumerate("qkv"):
        assert relmax(split_qkv(got, H)[i], split_qkv(want, H)[i]) < CEIL["bf16"][1], name
    assert relmax(r["colsum"].double().cpu(), want.sum(1)) < CEIL["bf16"][1]
