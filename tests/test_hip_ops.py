"""GPU parity tests of every C-ABI entry point against CPU restatements (torch fp32/fp64 math or oracle/).

Run on a real MI355X:  python -m pytest tests -m gpu -q
Tolerances are written next to each check.  bf16 MFMA kernels are compared with references computed in
fp64 FROM THE SAME bf16-ROUNDED INPUTS, so the only error left is fp32 accumulation order (~1e-6) plus, where the
output is bf16, one final rounding (2^-9 relative).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import quant_oracle  # noqa: E402
from oracle.vit_oracle import gelu_erf, layer_norm as ln_oracle, patchify as patchify_oracle  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    _ops.lib()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def dgelu64(x):
    x = x.double()
    return 0.5 * (1 + torch.erf(x / 2 ** 0.5)) + x * torch.exp(-0.5 * x * x) / (2 * np.pi) ** 0.5


# ---------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("rows,dim", [(1576, 192), (394, 768), (7, 1000), (5, 64)])
@pytest.mark.parametrize("odt", [torch.float32, torch.bfloat16])
def test_layernorm_fwd_bwd(ops, rows, dim, odt):
    x = torch.randn(rows, dim, generator=g(1)) * 2 + 0.5
    gam = torch.randn(dim, generator=g(2)) * 0.1 + 1
    bet = torch.randn(dim, generator=g(3)) * 0.1
    dy = torch.randn(rows, dim, generator=g(4))
    xr = x.double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    yr = ln_oracle(xr, gr, br)
    dyq = dy.to(odt).double()
    yr.backward(dyq)
    xd, gd, bd = x.cuda(), gam.cuda(), bet.cuda()
    y, mean, rstd = ops.layernorm_fwd(xd, dim, rows, dim, gd, bd, odt)
    tol = 2e-6 if odt == torch.float32 else 2.0 ** -8
    assert relerr(y.float(), yr) < tol
    add = torch.randn(rows, dim, generator=g(5))
    dx = torch.empty(rows, dim, device="cuda")
    dgam, dbet = ops.layernorm_bwd(dy.to(odt).cuda(), xd, dim, gd, mean, rstd, add.cuda(), dx, dim, rows, dim)
    assert relerr(dx, xr.grad + add.double()) < 5e-6
    assert relerr(dgam, gr.grad) < 5e-6
    assert relerr(dbet, br.grad) < 5e-6


def test_layernorm_strided_rows(ops):
    B, T, D = 6, 197, 192
    x = torch.randn(B, T, D, generator=g(1)).cuda()
    gam, bet = torch.ones(D).cuda(), torch.zeros(D).cuda()
    y, mean, rstd = ops.layernorm_fwd(x, T * D, B, D, gam, bet, torch.float32)       # the cls rows
    want = torch.nn.functional.layer_norm(x[:, 0].cpu(), (D,))
    assert relerr(y, want) < 2e-6


# ---------------------------------------------------------------- bf16 MFMA GEMMs
NT_SHAPES = [(1576, 192, 192), (1576, 576, 192), (394, 768, 768), (256, 1000, 768), (300, 45, 192), (129, 130, 200),
             (64, 17, 72), (1, 8, 8), (2560, 3072, 768),
             (6304, 2304, 768), (6304, 768, 3072)]        # batch 32: 225 tiles of 256^2 (8-phase from 192 tiles on) | 75: stays on 128^2


@pytest.mark.parametrize("M,N,K", NT_SHAPES)
def test_gemm_nt_bias_f32_out(ops, M, N, K):
    a, w, b = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(N, K, generator=g(2)) * K ** -0.5), torch.randn(N, generator=g(3))
    want = a.double() @ w.double().t() + b.double()
    wp = w.float().cuda()
    out = torch.empty(M, N, device="cuda")
    ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out, N)
    assert relerr(out, want) < 3e-6                      # fp32 accumulation of exact bf16 products
    out16 = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out16, N)
    assert relerr(out16.float(), want) < 2.0 ** -8        # + one bf16 rounding


@pytest.mark.parametrize("M,N,K", [(512, 512, 256), (130, 72, 64)])
def test_gelu_grad8_grid_holds_zero_and_one_exactly(ops, M, N, K):
    """the two most common values of gelu' must be grid points.  A saturated unit (pre-activation >> 0,
    gelu' = 1) gets code 226 and passes the gradient UNCHANGED; a dead unit (pre-activation << 0, gelu' = 0) gets code 26
    and leaks NOTHING: the consumer's output equals the plain product bit for bit, respectively is exactly zero."""
    a = bf(torch.randn(M, K, generator=g(1)))
    w = torch.zeros(N, K)
    b = torch.where(torch.arange(N) % 2 == 0, 30.0, -30.0)              # even columns saturated, odd columns dead
    g8 = torch.zeros(M, N, device="cuda", dtype=torch.uint8)
    act = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
    ops.linear_fwd(a.cuda(), M, K, w.cuda(), b.cuda(), act, N, epi=ops.EPI_GELU_GRAD8, out2=g8, ld_out2=N)
    assert bool((g8[:, 0::2] == 226).all()) and bool((g8[:, 1::2] == 26).all())
    # consumer: dx = (dy W2) * decode(codes); the codes tensor has the shape of dx, [M, K]
    dy, w2 = bf(torch.randn(M, N, generator=g(5))), bf(torch.randn(N, K, generator=g(6)) * N ** -0.5)
    codes = torch.where(torch.arange(K) % 2 == 0, 226, 26).to(torch.uint8).expand(M, K).contiguous()
    dx = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    plain = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    part = torch.zeros((M + 63) // 64, K, device="cuda")
    ops.linear_dx(dy.cuda(), M, N, w2.float().cuda(), dx, K, epi=ops.EPI_MUL8, aux=codes.cuda(), ld_aux=K, colsum_partial=part)
    ops.linear_dx(dy.cuda(), M, N, w2.float().cuda(), plain, K)
    assert torch.equal(dx[:, 0::2], plain[:, 0::2])                      # x 1.0 exactly
    assert bool((dx[:, 1::2] == 0).all())                                # x 0.0 exactly
    assert bool((part[:, 1::2] == 0).all())


# Every NT / TN kernel variant on shapes large enough to reach it (>= 2 tiles of 256, ragged M and N edges, K long
# enough for the 8-phase pipeline), all epilogues.  The automatic dispatch only picks the 256^2 kernels for >= 256
# tiles, which no unit-test shape has; mv_gemm_force_variant switches variants inside this one process.
@pytest.mark.parametrize("variant", [128, 2564, 2568])
@pytest.mark.parametrize("M,N,K", [(520, 300, 256), (777, 1000, 768), (256, 256, 128), (1030, 520, 3072)])
def test_gemm_nt_every_variant(ops, variant, M, N, K):
    from myrtle_vision.hip.lib import lib, check
    a, w, b = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(N, K, generator=g(2)) * K ** -0.5), torch.randn(N, generator=g(3)) * 0.1
    pre = a.double() @ w.double().t() + b.double()
    wp = w.float().cuda()
    check(lib().mv_gemm_force_variant(variant, 0), "force_variant")
    try:
        out = torch.empty(M, N, device="cuda")
        ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out, N)
        assert relerr(out, pre) < 3e-6
        ldn = (N + 7) & ~7
        act = torch.zeros(M, ldn, device="cuda", dtype=torch.bfloat16)
        h = torch.zeros(M, ldn, device="cuda", dtype=torch.bfloat16)
        ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), act, ldn, epi=ops.EPI_GELU, out2=h, ld_out2=ldn)
        assert relerr(h[:, :N].float(), pre) < 2.0 ** -8 and relerr(act[:, :N].float(), gelu_erf(pre)) < 2.0 ** -8
        res = torch.randn(M, N, generator=g(4))
        ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out, N, epi=ops.EPI_RESIDUAL, aux=res.cuda(), ld_aux=N)
        assert relerr(out, pre + res.double()) < 3e-6
        # dX entry point with DGELU (+ fc1 bias-gradient partial sums): contraction over N here
        if N % 8 == 0:
            dy, hh = bf(torch.randn(M, N, generator=g(5))), bf(torch.randn(M, K, generator=g(6)))
            want = (dy.double() @ w.double()) * dgelu64(hh)
            dx = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
            ops.linear_dx(dy.cuda(), M, N, wp, dx, K, epi=ops.EPI_DGELU, aux=hh.cuda(), ld_aux=K)
            assert relerr(dx.float(), want) < 2.0 ** -8
        # GELU_GRAD leaves gelu'(pre) for the backward pass; MUL consumes it (+ column-sum partials)
        gd = torch.zeros(M, ldn, device="cuda", dtype=torch.bfloat16)
        ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), act, ldn, epi=ops.EPI_GELU_GRAD, out2=gd, ld_out2=ldn)
        assert relerr(act[:, :N].float(), gelu_erf(pre)) < 2.0 ** -8 and relerr(gd[:, :N].float(), dgelu64(pre)) < 2.0 ** -8
        if N % 8 == 0:
            dy, gg = bf(torch.randn(M, N, generator=g(5))), bf(torch.randn(M, K, generator=g(8)))
            want = (dy.double() @ w.double()) * gg.double()
            dx = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
            part = torch.zeros((M + 63) // 64, K, device="cuda")
            ops.linear_dx(dy.cuda(), M, N, wp, dx, K, epi=ops.EPI_MUL, aux=gg.cuda(), ld_aux=K, colsum_partial=part)
            assert relerr(dx.float(), want) < 2.0 ** -8
            assert relerr(part.sum(0), want.sum(0)) < 3e-3
        # the 8-bit forms: gelu' as a code on the fixed grid (code - 26) * 0.005 (0 and 1 are grid points), and its consumer
        g8 = torch.full((M, ldn), 77, device="cuda", dtype=torch.uint8)
        act8 = torch.zeros(M, ldn, device="cuda", dtype=torch.bfloat16)
        ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), act8, ldn, epi=ops.EPI_GELU_GRAD8, out2=g8, ld_out2=ldn)
        assert torch.equal(act8[:, :N], act[:, :N])
        dec = (g8[:, :N].double().cpu() - 26) * 0.005
        assert float((dec - dgelu64(pre)).abs().max()) <= 0.5 * 0.005 + 2e-6
        if ldn > N:
            assert bool((g8[:, N:] == 77).all())                          # padding columns untouched
        if N % 8 == 0:
            dy = bf(torch.randn(M, N, generator=g(5)))
            codes = torch.randint(0, 256, (M, K), generator=g(9), dtype=torch.uint8)
            want = (dy.double() @ w.double()) * ((codes.double() - 26) * 0.005)
            dx = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
            part = torch.zeros((M + 63) // 64, K, device="cuda")
            ops.linear_dx(dy.cuda(), M, N, wp, dx, K, epi=ops.EPI_MUL8, aux=codes.cuda(), ld_aux=K, colsum_partial=part)
            assert relerr(dx.float(), want) < 2.0 ** -8
            assert relerr(part.sum(0), want.sum(0)) < 3e-3
        # a second launch is bit-identical (no race between DMA and fragment reads shows up as a flaky tile)
        out2 = torch.empty(M, N, device="cuda")
        for _ in range(3):
            ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out2, N, epi=ops.EPI_RESIDUAL, aux=res.cuda(), ld_aux=N)
            assert torch.equal(out, out2)
    finally:
        check(lib().mv_gemm_force_variant(0, 0), "force_variant")


@pytest.mark.parametrize("M,N,K", [(520, 300, 128), (777, 2304, 256), (1030, 2304, 768), (2048, 2304, 3072), (9000, 2304, 768),
                                   (4859, 3584, 512)])
def test_gemm_nt_8phase_optional_features(ops, M, N, K):
    """Round 4: the 8-phase kernel's column-band tile order (a different workgroup -> tile map; force 3102 = bands on, 3100 = off)
    against the plain forced kernel (2568 = the default feature set) BIT FOR BIT -- the map changes no arithmetic -- on 2, 4, 12 and
    48 K-tiles, 9 tile columns (bands of 3), ragged edges, a half-item tail, all epilogue families.  Outputs start as NaN: a tile
    the band map skipped, or reached twice, cannot pass.  (A second optional feature of the round, an L2 prefetch of the operand
    lines, passed this test too and was removed for speed: DESIGN finding 38.)"""
    from myrtle_vision.hip.lib import lib, check
    a, w, b = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(N, K, generator=g(2)) * K ** -0.5), torch.randn(N, generator=g(3)) * 0.1
    ad, wd, bd = a.cuda(), w.float().cuda(), b.cuda()
    res = torch.randn(M, N, generator=g(4)).cuda()
    ldn = (N + 15) & ~15
    dy = bf(torch.randn(M, N, generator=g(5))).cuda() if N % 8 == 0 else None
    codes = torch.randint(0, 256, (M, (K + 15) & ~15), generator=g(9), dtype=torch.uint8).cuda()

    def run():
        nan32 = lambda *s: torch.full(s, float("nan"), device="cuda")
        nan16 = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=torch.bfloat16)
        o32 = nan32(M, N); ops.linear_fwd(ad, M, K, wd, bd, o32, N)
        o16 = nan16(M, ldn); ops.linear_fwd(ad, M, K, wd, bd, o16, ldn)
        r32 = nan32(M, N); ops.linear_fwd(ad, M, K, wd, bd, r32, N, epi=ops.EPI_RESIDUAL, aux=res, ld_aux=N)
        act, g8 = nan16(M, ldn), torch.full((M, ldn), 77, device="cuda", dtype=torch.uint8)
        ops.linear_fwd(ad, M, K, wd, bd, act, ldn, epi=ops.EPI_GELU_GRAD8, out2=g8, ld_out2=ldn)
        outs = [o32, o16[:, :N], r32, act[:, :N], g8[:, :N]]
        if dy is not None:
            dx = nan16(M, K); part = torch.zeros((M + 63) // 64, K, device="cuda")
            ops.linear_dx(dy, M, N, wd, dx, K, epi=ops.EPI_MUL8, aux=codes, ld_aux=codes.shape[1], colsum_partial=part)
            outs += [dx, part]
        return outs

    got = {}
    # round 4: IEEE-half output (MV_EPI_NONE) = the fp32 result rounded once, on the 8-phase and on the 128-tile kernels
    for variant in (2568, 128):
        check(lib().mv_gemm_force_variant(variant, 0), "force_variant")
        try:
            o32 = torch.full((M, N), float("nan"), device="cuda"); ops.linear_fwd(ad, M, K, wd, bd, o32, N)
            o16 = torch.full((M, ldn), float("nan"), device="cuda", dtype=torch.float16)
            check(lib().mv_gemm_nt_bf16(ad.data_ptr(), K, ops.prepared_weight(wd).w.data_ptr(), ops.prepared_weight(wd).ldw,
                                        o16.data_ptr(), ldn, 3, M, N, K, bd.data_ptr(), ops.EPI_NONE, None, 0, 0, None, 0,
                                        torch.cuda.current_stream().cuda_stream), "gemm_nt_bf16(f16 out)")
            # one rounding of the fp32 result: within half an ulp of half everywhere, and the same value as torch's cast except
            # on exact ties (about 2^-13 of random data: the hardware conversion and torch break them differently)
            got16 = o16[:, :N].float()
            assert bool(((got16 - o32).abs() <= o32.abs() * 2.0 ** -11 + 2.0 ** -24).all())
            assert float((o16[:, :N] != o32.half()).float().mean()) < 2e-4
        finally:
            check(lib().mv_gemm_force_variant(0, 0), "force_variant")
    for variant in (2568, 3100, 3102):
        check(lib().mv_gemm_force_variant(variant, 0), "force_variant")
        try:
            got[variant] = run()
            again = run()                                                  # a second launch: bit-identical (no race)
            for x, y in zip(got[variant], again):
                assert torch.equal(x, y)
        finally:
            check(lib().mv_gemm_force_variant(0, 0), "force_variant")
    pre = (ad.float() @ wd.t()).double().cpu() + b.double()
    assert relerr(got[2568][0], pre) < 1e-5 and not torch.isnan(got[2568][1].float()).any()
    for variant in (3100, 3102):
        for i, (x, y) in enumerate(zip(got[variant], got[2568])):
            assert torch.equal(x, y), (variant, i)


@pytest.mark.parametrize("M,N,K", [(4859, 3584, 512), (4864, 3584, 768)])
def test_gemm_nt_tail_split(ops, M, N, K):
    """266 tiles of 256x256 on 256 CUs: the 10 tail tiles run as 20 half items (128x256, quadrant-row 0 of the pipeline
    only) -- every epilogue must give the same result as whole tiles, including the ragged last row block."""
    from myrtle_vision.hip.lib import lib
    a, w, b = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(N, K, generator=g(2)) * K ** -0.5), torch.randn(N, generator=g(3)) * 0.1
    ad, wd = a.cuda(), w.float().cuda()
    pre = (ad.float() @ wd.t()).double().cpu() + b.double()        # fp32 reference of exact bf16 products (GPU matmul)
    out = torch.empty(M, N, device="cuda")
    ops.linear_fwd(ad, M, K, wd, b.cuda(), out, N)
    assert relerr(out, pre) < 1e-5
    res = torch.randn(M, N, generator=g(4))
    ops.linear_fwd(ad, M, K, wd, b.cuda(), out, N, epi=ops.EPI_RESIDUAL, aux=res.cuda(), ld_aux=N)
    assert relerr(out, pre + res.double()) < 1e-5
    act = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    h = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.linear_fwd(ad, M, K, wd, b.cuda(), act, N, epi=ops.EPI_GELU, out2=h, ld_out2=N)
    assert relerr(h.float(), pre) < 2.0 ** -8 and relerr(act.float(), gelu_erf(pre)) < 2.0 ** -8
    # the same product from the ring kernel (whole tiles only): identical up to fp32 summation order
    lib().mv_gemm_force_variant(2564, 0)
    try:
        out_ring = torch.empty(M, N, device="cuda")
        ops.linear_fwd(ad, M, K, wd, b.cuda(), out_ring, N, epi=ops.EPI_RESIDUAL, aux=res.cuda(), ld_aux=N)
    finally:
        lib().mv_gemm_force_variant(0, 0)
    assert relerr(out, out_ring.double().cpu()) < 2e-6
    # DGELU through the dX entry point: C[M, K2] with K2 = 3584 columns, contraction over 512/768
    dy = bf(torch.randn(M, K, generator=g(5)))
    hh = bf(torch.randn(M, N, generator=g(6)))
    w2 = bf(torch.randn(K, N, generator=g(7)) * K ** -0.5)         # nn.Linear weight [out=K, in=N]: dX = dy @ w2
    want = (dy.cuda().float() @ w2.cuda().float()).double().cpu() * dgelu64(hh)
    dx = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    part = torch.zeros((M + 63) // 64, N, device="cuda")
    ops.linear_dx(dy.cuda(), M, K, w2.float().cuda(), dx, N, epi=ops.EPI_DGELU, aux=hh.cuda(), ld_aux=N, colsum_partial=part)
    assert relerr(dx.float(), want) < 2.0 ** -8
    assert relerr(part.sum(0), want.sum(0)) < 2e-3


def test_gemm_nt_epilogues(ops):
    M, N, K = 1576, 768, 192
    a, w, b = bf(torch.randn(M, K, generator=g(1))), bf(torch.randn(N, K, generator=g(2)) * K ** -0.5), torch.randn(N, generator=g(3)) * 0.1
    pre = a.double() @ w.double().t() + b.double()
    wp = w.float().cuda()
    # GELU: C = gelu(pre) bf16, out2 = pre bf16
    act = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    h = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), act, N, epi=ops.EPI_GELU, out2=h, ld_out2=N)
    assert relerr(h.float(), pre) < 2.0 ** -8
    assert relerr(act.float(), gelu_erf(pre)) < 2.0 ** -8
    # RESIDUAL: fp32
    res = torch.randn(M, N, generator=g(4))
    out = torch.empty(M, N, device="cuda")
    ops.linear_fwd(a.cuda(), M, K, wp, b.cuda(), out, N, epi=ops.EPI_RESIDUAL, aux=res.cuda(), ld_aux=N)
    assert relerr(out, pre + res.double()) < 3e-6
    # DGELU via the dX entry point: out[M,K] = (dy[M,N] @ W[N,K]) * gelu'(hh[M,K])
    dy = bf(torch.randn(M, N, generator=g(5)))
    hh = bf(torch.randn(M, K, generator=g(6)))
    want = (dy.double() @ w.double()) * dgelu64(hh)
    dx = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    ops.linear_dx(dy.cuda(), M, N, wp, dx, K, epi=ops.EPI_DGELU, aux=hh.cuda(), ld_aux=K)
    assert relerr(dx.float(), want) < 2.0 ** -8


def test_gemm_nt_embed_epilogue(ops):
    B, npatch, D, pd = 3, 196, 192, 768
    a, w, b = bf(torch.randn(B * npatch, pd, generator=g(1))), bf(torch.randn(D, pd, generator=g(2)) * pd ** -0.5), torch.randn(D, generator=g(3))
    pos = torch.randn(npatch + 1, D, generator=g(4))
    x = torch.full((B, npatch + 1, D), 7.0, device="cuda")
    ops.linear_fwd(a.cuda(), B * npatch, pd, w.float().cuda(), b.cuda(), x, D, epi=ops.EPI_EMBED, aux=pos.cuda(), ld_aux=D, aux_i=npatch)
    want = (a.double() @ w.double().t() + b.double()).view(B, npatch, D) + pos[1:].double()
    assert relerr(x[:, 1:], want) < 3e-6
    assert (x[:, 0] == 7.0).all()                          # cls rows untouched


TN_SHAPES = [(1576, 192, 576), (1600, 192, 576), (4096, 200, 136), (1576, 768, 192), (5000, 768, 768), (256, 48, 768), (100, 136, 200), (63, 8, 8),
             (20000, 3072, 768), (9456, 768, 2304), (19700, 3072, 768), (4097, 768, 768),   # these three: ragged contractions
             (6304, 768, 768), (6304, 768, 2304)]   # batch 32: 9 tiles x 13 splits -> the 128-tile kernel | 27 x 9 -> the ring
                                                                                    # (197 x 48 / x 100 rows): ring + tail


@pytest.mark.parametrize("Kc,M,N", TN_SHAPES)
def test_gemm_tn_dw_and_colsum(ops, Kc, M, N):
    dy, x = bf(torch.randn(Kc, M, generator=g(1))), bf(torch.randn(Kc, N, generator=g(2)))
    want = dy.double().t() @ x.double()
    dw, db = ops.linear_dw(dy.cuda(), x.cuda(), Kc, M, N)
    assert relerr(dw, want) < 3e-6
    assert relerr(db, dy.double().sum(0)) < 3e-6


@pytest.mark.parametrize("variant", [128, 256])
@pytest.mark.parametrize("Kc,M,N", [(4096, 520, 300 // 4 * 4 + 4), (6400, 768, 768), (2080, 264, 1000), (9984, 776, 520)])
def test_gemm_tn_every_variant(ops, variant, Kc, M, N):
    from myrtle_vision.hip.lib import lib, check
    dy, x = bf(torch.randn(Kc, M, generator=g(1))), bf(torch.randn(Kc, N, generator=g(2)))
    want = dy.double().t() @ x.double()
    check(lib().mv_gemm_force_variant(0, variant), "force_variant")
    try:
        dw, db = ops.linear_dw(dy.cuda(), x.cuda(), Kc, M, N)
        assert relerr(dw, want) < 3e-6
        assert relerr(db, dy.double().sum(0)) < 3e-6
        dw2, _ = ops.linear_dw(dy.cuda(), x.cuda(), Kc, M, N)
        assert torch.equal(dw, dw2)                                   # deterministic split-K reduce
    finally:
        check(lib().mv_gemm_force_variant(0, 0), "force_variant")


def test_misaligned_leading_dimension_is_rejected(ops):
    dy, x = bf(torch.randn(100, 130)), bf(torch.randn(100, 200))
    with pytest.raises(RuntimeError, match="not aligned"):
        ops.linear_dw(dy.cuda(), x.cuda(), 100, 130, 200)


def test_gemm_tn_padded_rows(ops):
    # class dim 45 padded to 48 with zero columns (ld_dy = 48): only the first 45 output rows exist
    Kc, C, D = 256, 45, 192
    dy = torch.zeros(Kc, 48)
    dy[:, :C] = torch.randn(Kc, C, generator=g(1))
    dy, x = bf(dy), bf(torch.randn(Kc, D, generator=g(2)))
    dw, db = ops.linear_dw(dy.cuda(), x.cuda(), Kc, C, D, ld_dy=48)
    assert dw.shape == (C, D)
    assert relerr(dw, dy[:, :C].double().t() @ x.double()) < 3e-6
    assert relerr(db, dy[:, :C].double().sum(0)) < 3e-6


# ---------------------------------------------------------------- fp32 strided GEMM
def test_gemm_f32_linear_forms(ops):
    M, N, K = 333, 77, 130
    x, w, b = torch.randn(M, K, generator=g(1)), torch.randn(N, K, generator=g(2)), torch.randn(N, generator=g(3))
    out = torch.empty(M, N, device="cuda")
    ops.linear_fwd(x.cuda(), M, K, w.cuda(), b.cuda(), out, N)
    assert relerr(out, x.double() @ w.double().t() + b.double()) < 2e-6
    dy = torch.randn(M, N, generator=g(4))
    dx = torch.empty(M, K, device="cuda")
    ops.linear_dx(dy.cuda(), M, N, w.cuda(), dx, K)
    assert relerr(dx, dy.double() @ w.double()) < 2e-6
    dw, db = ops.linear_dw(dy.cuda(), x.cuda(), M, N, K)
    assert relerr(dw, dy.double().t() @ x.double()) < 2e-6
    assert relerr(db, dy.double().sum(0)) < 2e-6


@pytest.mark.parametrize("M,N,K", [(333, 77, 130), (1024, 768, 768), (1576, 3072, 768), (1000, 768, 3072), (197, 197, 64),
                                   (197, 64, 197), (130, 260, 19), (516, 388, 48)])
def test_gemm_f32_mfma_is_bitwise_the_fma_chain(ops, M, N, K):
    """The f32-input MFMA kernel (v_mfma_f32_16x16x4_f32) computes, per output, the same k-ordered fmaf chain as the FMA
    kernel: every Linear form (forward / dX / dW: three stride patterns), the batched attention products and the fused
    epilogues must agree BIT FOR BIT, and both must match fp64."""
    from myrtle_vision.hip.lib import lib
    x, w, b = torch.randn(M, K, generator=g(1)).cuda(), torch.randn(N, K, generator=g(2)).cuda(), torch.randn(N, generator=g(3)).cuda()
    dy = torch.randn(M, N, generator=g(4)).cuda()
    res = torch.randn(M, N, generator=g(5)).cuda()

    def run_all():
        outs = []
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N); outs.append(o)
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_RESIDUAL, aux=res, ld_aux=N); outs.append(o)
        o, h = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_GELU, out2=h, ld_out2=N); outs += [o, h]
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K); outs.append(o)
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K, epi=ops.EPI_DGELU, aux=x, ld_aux=K); outs.append(o)
        dw, db = ops.linear_dw(dy, x, M, N, K); outs += [dw, db]
        return outs

    prev = ops.set_f32_gemm("mfma")                  # this test is about mv_gemm_f32, not the bf16x6 products
    try:
        lib().mv_gemm_f32_force_fma(1)
        fma = run_all()
        lib().mv_gemm_f32_force_fma(2)               # matrix cores, generic kernel only
        generic = run_all()
        lib().mv_gemm_f32_force_fma(0)
        mfma = run_all()                             # matrix cores, fast kernel where the shape allows
    finally:
        lib().mv_gemm_f32_force_fma(0)
        ops.set_f32_gemm(prev)
    for i, (a, c, d) in enumerate(zip(fma, mfma, generic)):
        assert torch.equal(a, c) and torch.equal(a, d), i
    tol = 2e-6 if max(M, N, K) <= 1024 else 6e-6        # a chain of K fp32 roundings (3.5e-7 sum|ab| at K = 4096)
    assert relerr(mfma[0], x.double().cpu() @ w.double().cpu().t() + b.double().cpu()) < tol
    assert relerr(mfma[4], dy.double().cpu() @ w.double().cpu()) < tol
    assert relerr(mfma[6], dy.double().cpu().t() @ x.double().cpu()) < tol


def test_split3_bf16_pieces_reconstruct_fp32(ops):
    """mv_split3_bf16: the three bf16 pieces sum back to the fp32 value to 2^-26 |x| (exactly, for most values), and the six
    segments come out in the documented order for both roles and both layouts."""
    rows, cols = 37, 64
    x = (torch.randn(rows, cols + 4, generator=g(1)) * torch.logspace(-12, 12, cols + 4)).cuda()
    for role, order in ((0, (0, 0, 1, 0, 1, 2)), (1, (0, 1, 0, 2, 1, 0))):
        side = ops.split3(x, rows, cols, cols + 4, role).view(rows, 6, cols)
        stacked = ops.split3(x, rows, cols, cols + 4, role, stack=True).view(6, rows, cols)
        assert torch.equal(side.permute(1, 0, 2), stacked)
        pieces = {}
        for s_, pi in enumerate(order):
            pieces.setdefault(pi, stacked[s_])
            assert torch.equal(pieces[pi], stacked[s_])
        total = pieces[0].double() + pieces[1].double() + pieces[2].double()
        xr = x[:, :cols].double()
        assert ((total - xr).abs() <= xr.abs() * 2.0 ** -26).all()
        assert torch.equal(pieces[0], x[:, :cols].to(torch.bfloat16))


@pytest.mark.parametrize("M,N,K", [(394, 192, 192), (1600, 768, 768), (1600, 3072, 768), (1024, 768, 3072), (4096, 2304, 768)])
def test_gemm_f32_bf16x6_is_fp32_accurate(ops, M, N, K):
    """The bf16x6 products (three-piece bf16 split, six pairings, one bf16 MFMA product) against fp64 and against the bit-exact
    fmaf-chain kernel: forward (+bias, +residual, +GELU with kept pre-activation), dX (+GELU'), dW/db.  Error bound: the
    2^-25 of the dropped cross terms plus fp32 accumulation, i.e. what an fp32 product of the same length carries."""
    x, w, b = torch.randn(M, K, generator=g(1)).cuda(), torch.randn(N, K, generator=g(2)).cuda(), torch.randn(N, generator=g(3)).cuda()
    dy, res = torch.randn(M, N, generator=g(4)).cuda(), torch.randn(M, N, generator=g(5)).cuda()

    def run_all():
        outs = []
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N); outs.append(o)
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_RESIDUAL, aux=res, ld_aux=N); outs.append(o)
        o, h = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_GELU, out2=h, ld_out2=N); outs += [o, h]
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K); outs.append(o)
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K, epi=ops.EPI_DGELU, aux=x, ld_aux=K); outs.append(o)
        dw, db = ops.linear_dw(dy, x, M, N, K); outs += [dw, db]
        return outs

    assert ops.set_f32_gemm("bf16x6") in ("bf16x6", "mfma")
    x6 = run_all()
    prev = ops.set_f32_gemm("mfma")
    try:
        chain = run_all()
    finally:
        ops.set_f32_gemm("bf16x6")
    ref64 = [x.double() @ w.double().t() + b.double(), None, None, None, dy.double() @ w.double(), None,
             dy.double().t() @ x.double(), dy.double().sum(0)]
    for i, (a, c) in enumerate(zip(x6, chain)):
        assert relerr(a, c.double()) < 5e-6, i                     # the two fp32 paths agree to fp32 accuracy
        if ref64[i] is not None:
            # and bf16x6 is at least as close to fp64 as twice the fmaf chain's own error
            assert relerr(a, ref64[i]) <= max(2.0 * relerr(c, ref64[i]), 3e-7), i
    # inside a split_scope the dX and dW products share dY's split: same bits as without sharing
    with ops.split_scope():
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K)
        dw, db = ops.linear_dw(dy, x, M, N, K)
    assert torch.equal(o, x6[4]) and torch.equal(dw, x6[6])
    # (the bias gradient comes from the split pass when the split is made by the dW call, from the colsum kernel when the
    # split is found in the scope's memo: two summation orders of the same column sums)
    assert relerr(db, x6[7].double()) < 2e-6 and relerr(db, dy.double().sum(0)) < 2e-6
    # weights are re-split when the parameter changes in place
    w.mul_(2.0)
    o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N)
    assert relerr(o, x.double() @ w.double().t() + b.double()) < 4e-6


@pytest.mark.parametrize("M,D,Hd", [(512, 768, 3072), (1024, 256, 512), (2048, 384, 768)])
@pytest.mark.parametrize("nseg", [3, 6])
def test_split_output_epilogues_equal_gemm_then_split(ops, M, D, Hd, nseg):
    """MV_EPI_SPLIT_GELU / MV_EPI_SPLIT_DGELU (round 4): fc1 and fc2-dX of the split-operand modes with the pieces of gelu(h) /
    (dY W2) gelu'(h) leaving the GEMM epilogue -- against the two passes they replace (fp32 GEMM output, then mv_split*_bf16_ex with
    op 1 / 2): the same erf and piece arithmetic on the epilogue's own fp32 accumulator (the pieces of gelu(h) are bit-identical to
    a split pass over the h it wrote), values against the two-pass path to fp32 rounding and against fp64 to the mode's accuracy,
    bias-gradient column sums included."""
    x, w1, b1 = torch.randn(M, D, generator=g(1)).cuda(), (torch.randn(Hd, D, generator=g(2)) * D ** -0.5).cuda(), (0.1 * torch.randn(Hd, generator=g(3))).cuda()
    w2, dy = (torch.randn(D, Hd, generator=g(4)) * Hd ** -0.5).cuda(), torch.randn(M, D, generator=g(5)).cuda()
    with ops.segments(nseg):
        assert ops.nt_split_ok(M, Hd, D)
        y6 = ops.split_ex(x, M, D)
        h_ref = torch.empty(M, Hd, device="cuda"); ops.nt_x6(y6, w1, "fwd", M, h_ref, bias=b1)
        h = torch.full((M, Hd), float("nan"), device="cuda")
        a6 = ops.nt_x6_gelu_split(y6, w1, M, h, bias=b1)
        # (the plain product may run K-split for so few tiles: another summation order of the same fp32 product)
        assert relerr(h, h_ref.double()) < 2e-6
        assert torch.equal(a6, ops.split_ex(h, M, Hd, op=1))               # the pieces of gelu(h) of exactly the h it wrote
        d6 = ops.split_ex(dy, M, D)
        dh = torch.empty(M, Hd, device="cuda"); ops.nt_x6(d6, w2, "dx", M, dh)
        db_ref = torch.empty(Hd, device="cuda")
        dh6_ref = ops.split_ex(dh, M, Hd, op=2, h=h, colsum_out=db_ref)
        db = torch.empty(Hd, device="cuda")
        dh6 = ops.nt_x6_dgelu_split(d6, w2, M, h, db)
        npc = 2 if nseg == 3 else 3
        val = lambda t: sum(t[:, i * Hd:(i + 1) * Hd].double() for i in ((0, 2) if nseg == 3 else (0, 2, 5)))
        # (two pieces carry a value to 2^-17: the reconstructions of two fp32 values that differ in their last bits differ by that)
        assert relerr(val(dh6), val(dh6_ref)) < (2e-5 if nseg == 3 else 2e-6) and torch.equal(dh6[:, :Hd], dh6[:, Hd:2 * Hd])
        assert relerr(db, db_ref.double()) < 2e-6
        # the values themselves, against fp64
        hd = x.double() @ w1.double().t() + b1.double()
        gel = torch.nn.functional.gelu(hd)
        assert relerr(val(a6), gel) < (2e-5 if nseg == 3 else 2e-6)
        hg = hd.clone().requires_grad_(True)
        (dgel,) = torch.autograd.grad(torch.nn.functional.gelu(hg).sum(), hg)
        assert relerr(val(dh6), (dy.double() @ w2.double()) * dgel) < (3e-5 if nseg == 3 else 3e-6)
        # a large enough grid takes the plain one-launch product on both sides: then everything is bit-identical


@pytest.mark.parametrize("rows,dim", [(394, 192), (1000, 768), (37, 1024), (513, 64)])
def test_layernorm_fwd_split_equals_layernorm_then_split(ops, rows, dim):
    """mv_layernorm_fwd_split (round 4): LayerNorm whose output leaves as the bf16 pieces of the split-operand products -- bit for
    bit what mv_layernorm_fwd (fp32) followed by the split pass writes, statistics included, for three and six segments; the rows
    behind the last one (the dW product walks whole 32-row stages) are zero."""
    x = torch.randn(rows, dim, generator=g(1)).cuda() * 2 + 0.3
    gm, bt = (1 + 0.1 * torch.randn(dim, generator=g(2))).cuda(), (0.1 * torch.randn(dim, generator=g(3))).cuda()
    y, mean, rstd = ops.layernorm_fwd(x, dim, rows, dim, gm, bt, torch.float32)
    for nseg in (6, 3):
        with ops.segments(nseg):
            want = ops.split_ex(y, rows, dim)
            got, m2, r2 = ops.layernorm_fwd_split(x, dim, rows, dim, gm, bt)
        assert got.shape == (rows, nseg * dim) and torch.equal(got, want)
        assert torch.equal(m2, mean) and torch.equal(r2, rstd)
        pad = got.storage_offset() + got.numel()
        full = torch.empty(0, dtype=torch.bfloat16, device="cuda").set_(got.untyped_storage())
        assert not full[pad:((rows + 31) // 32) * 32 * nseg * dim].any()


@pytest.mark.parametrize("M,N,K", [(394, 192, 192), (1600, 768, 768), (1600, 3072, 768), (1024, 768, 3072), (4096, 2304, 768)])
def test_gemm_f32_bf16x3_is_2e16_accurate(ops, M, N, K):
    """The bf16x3 products (``ops.segments(3)``: two bf16 pieces per operand, pairings a0 b0 + a0 b1 + a1 b0 in ONE bf16 MFMA
    product over 3 K) against fp64: forward (+bias, +residual, +GELU), dX (+GELU'), dW / db.  Error model: a piece is an 8-bit
    significand, so the dropped terms (a1 b1, the third pieces) are <= 2^-16 |a||b| per product -- 256x below a plain bf16 product
    -- and they add up like rounding noise over the contraction.  Bounds: 2e-5 of max|C| (a plain bf16 product of these
    operands measures ~3e-3), and the pieces themselves are exact: p0 + p1 == x to 2^-17 |x|."""
    x, w, b = torch.randn(M, K, generator=g(1)).cuda(), torch.randn(N, K, generator=g(2)).cuda(), torch.randn(N, generator=g(3)).cuda()
    dy, res = torch.randn(M, N, generator=g(4)).cuda(), torch.randn(M, N, generator=g(5)).cuda()
    with ops.segments(3):
        s2 = ops.split3(x, M, K, K, 0)
        assert s2.shape == (M, 3 * K)
        p0, p0b, p1 = s2[:, :K].float(), s2[:, K:2 * K].float(), s2[:, 2 * K:].float()
        assert torch.equal(p0, p0b) and torch.equal(p0, x.bfloat16().float())
        assert float(((p0 + p1) - x).abs().max() / x.abs().max()) < 2.0 ** -16
        r2 = ops.split3(x, M, K, K, 1)                                  # right-operand order: p0 p1 p0
        assert torch.equal(r2[:, :K], s2[:, :K]) and torch.equal(r2[:, K:2 * K], s2[:, 2 * K:]) and torch.equal(r2[:, 2 * K:], s2[:, :K])
        outs = []
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N); outs.append(o)
        o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_RESIDUAL, aux=res, ld_aux=N); outs.append(o)
        o, h = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
        ops.linear_fwd(x, M, K, w, b, o, N, epi=ops.EPI_GELU, out2=h, ld_out2=N); outs += [o, h]
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K); outs.append(o)
        o = torch.empty(M, K, device="cuda"); ops.linear_dx(dy, M, N, w, o, K, epi=ops.EPI_DGELU, aux=x, ld_aux=K); outs.append(o)
        with ops.split_scope():
            dw, db = ops.linear_dw(dy, x, M, N, K); outs += [dw, db]
    y64 = x.double() @ w.double().t() + b.double()
    gelu = torch.nn.functional.gelu
    dx64 = dy.double() @ w.double()
    xd = x.double().requires_grad_(True)
    (dgelu,) = torch.autograd.grad(gelu(xd).sum(), xd)
    ref64 = [y64, y64 + res.double(), gelu(y64), y64, dx64, dx64 * dgelu, dy.double().t() @ x.double(), dy.double().sum(0)]
    worst = 0.0
    for i, (a, r) in enumerate(zip(outs, ref64)):
        e = relerr(a, r)
        worst = max(worst, e)
        assert e < 2e-5, (i, e)
    # the scope is per call: outside it the same calls are bf16x6 again (and far tighter)
    o = torch.empty(M, N, device="cuda"); ops.linear_fwd(x, M, K, w, b, o, N)
    assert relerr(o, y64) < 2e-6 and worst > relerr(o, y64)


def test_attention_materialised_fp32_mfma_equals_fma(ops):
    from myrtle_vision.hip.lib import lib
    B, N, H, dh = 2, 197, 3, 64
    qkv = torch.randn(B, N, 3 * H * dh, generator=g(1)).cuda()
    dout = torch.randn(B, N, H * dh, generator=g(2)).cuda()

    def run():
        probs = ops.attention_probs_fp32(qkv, B, N, H, dh, dh ** -0.5)
        return probs, ops.attention_pv_fp32(probs, qkv, B, N, H, dh), ops.attention_bwd_fp32(probs, qkv, dout, B, N, H, dh, dh ** -0.5)

    lib().mv_gemm_f32_force_fma(1)
    try:
        a = run()
    finally:
        lib().mv_gemm_f32_force_fma(0)
    for u, v in zip(a, run()):
        assert torch.equal(u, v)


# ---------------------------------------------------------------- attention
def attn_ref(qkv, H, scale):
    B, N, _ = qkv.shape
    dh = qkv.shape[2] // (3 * H)
    q, k, v = qkv.double().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    p = ((q @ k.transpose(-2, -1)) * scale).softmax(-1)
    return (p @ v).transpose(1, 2).reshape(B, N, H * dh), p


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (1, 257, 2), (3, 50, 1), (1, 17, 12), (2, 216, 2), (1, 208, 1), (1, 288, 1), (1, 300, 2)])
def test_attention_fused_fwd_bwd(ops, B, N, H):
    scale = 64 ** -0.5
    qkv = bf(torch.randn(B, N, 3 * H * 64, generator=g(1)) * 1.5)
    dout = bf(torch.randn(B, N, H * 64, generator=g(2)))
    ref_in = qkv.double().requires_grad_(True)
    want, _ = attn_ref(ref_in, H, scale)
    want.backward(dout.double())
    out, lse = ops.attention_fwd(qkv.cuda(), B, N, H, scale)
    # P is rounded to bf16 before P.V (2^-9 per element, averaged over keys) and the output once more
    assert relerr(out.float(), want) < 1.5e-2
    q, k, _ = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    lse_ref = torch.logsumexp((q @ k.transpose(-2, -1)) * scale, dim=-1)
    assert float((lse.cpu().double() - lse_ref).abs().max()) < 1e-4
    # every forward kernel (auto picked one): one query tile per wave pass, query-tile PAIRS sharing every K / V^T fragment
    # (N <= 224), and the 13-key-tile form with three workgroups per CU (N <= 208) -- the same MFMA sequence per query row
    # in all three, so the same bits (a variant that cannot take the length falls back)
    from myrtle_vision.hip.lib import lib
    for variant in (1, 2, 3):
        lib().mv_attention_fwd_force(variant)
        try:
            out_v, lse_v = ops.attention_fwd(qkv.cuda(), B, N, H, scale)
        finally:
            lib().mv_attention_fwd_force(0)
        assert relerr(out_v.float(), want) < 1.5e-2, variant
        assert torch.equal(out_v, out) and torch.equal(lse_v, lse), variant
    part = torch.full((B, 3 * H * 64), float("nan"), device="cuda")
    dqkv = ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale, colsum=part)
    got, ref = dqkv.float().cpu().view(B, N, 3, H, 64), ref_in.grad.view(B, N, 3, H, 64)
    for i, name in enumerate("qkv"):
        assert relerr(got[:, :, i], ref[:, :, i]) < 3e-2, name
    # fused per-image column sums (to_qkv bias-gradient partials): the sums of what the kernel wrote, before bf16 rounding
    sums = dqkv.float().sum(1).cpu()                                      # [B, 3*H*64] from the rounded outputs
    assert relerr(part.cpu(), sums) < 5e-3
    assert relerr(part.cpu().double(), ref_in.grad.sum(1)) < 3e-2
    dq2 = ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale)           # colsum is optional
    assert torch.equal(dq2, dqkv)
    # every backward kernel that takes this length (auto picked one of them above)
    from myrtle_vision.hip.lib import lib
    for variant in [v for v, nmax in ((4, 208), (5, 208), (2, 288), (8, 320)) if N <= nmax]:
        lib().mv_attention_bwd_force(variant)
        try:
            part2 = torch.full((B, 3 * H * 64), float("nan"), device="cuda")
            got2 = ops.attention_bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale, colsum=part2).float().cpu().view(B, N, 3, H, 64)
        finally:
            lib().mv_attention_bwd_force(0)
        for i, name in enumerate("qkv"):
            assert relerr(got2[:, :, i], ref[:, :, i]) < 3e-2, (variant, name)
        assert relerr(part2.cpu().double(), ref_in.grad.sum(1)) < 3e-2, variant


@pytest.mark.parametrize("B,N,H,dh", [(2, 197, 3, 64), (1, 40, 2, 32)])
def test_attention_materialised_fp32(ops, B, N, H, dh):
    scale = dh ** -0.5
    qkv = torch.randn(B, N, 3 * H * dh, generator=g(1))
    dout = torch.randn(B, N, H * dh, generator=g(2))
    ref_in = qkv.double().requires_grad_(True)
    want, p_ref = attn_ref(ref_in, H, scale)
    want.backward(dout.double())
    probs = ops.attention_probs_fp32(qkv.cuda(), B, N, H, dh, scale)
    assert relerr(probs, p_ref) < 5e-6
    out = ops.attention_pv_fp32(probs, qkv.cuda(), B, N, H, dh)
    assert relerr(out, want) < 5e-6
    dqkv = ops.attention_bwd_fp32(probs, qkv.cuda(), dout.cuda(), B, N, H, dh, scale)
    assert relerr(dqkv, ref_in.grad) < 2e-5


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (1, 257, 2), (3, 50, 1), (1, 17, 12), (2, 208, 2), (1, 272, 1)])
def test_attention_fused_fp32_forward(ops, B, N, H):
    """mv_attention_fwd_f32 (exact fp32 arithmetic on the f32 MFMA, no probabilities kept) against fp64 and against the
    materialised fp32 path it replaces under no_grad: same products, only the summation order differs."""
    scale = 64 ** -0.5
    qkv = torch.randn(B, N, 3 * H * 64, generator=g(1)) * 1.5
    want, _ = attn_ref(qkv, H, scale)
    out = ops.attention_fwd_f32(qkv.cuda(), B, N, H, scale)
    assert out.shape == (B, N, H * 64) and out.dtype == torch.float32
    assert relerr(out, want) < 2e-6
    probs = ops.attention_probs_fp32(qkv.cuda(), B, N, H, 64, scale)
    mat = ops.attention_pv_fp32(probs, qkv.cuda(), B, N, H, 64)
    assert relerr(out, mat.double().cpu()) < 2e-6
    # a spiked score (softmax max far above the rest) and a second launch (deterministic)
    qkv2 = qkv.clone()
    qkv2[0, 3, :64] *= 30.0
    want2, _ = attn_ref(qkv2, H, scale)
    out2 = ops.attention_fwd_f32(qkv2.cuda(), B, N, H, scale)
    # (scores of ~ +-300 here: one fp32 ulp of the score is 3e-5 absolute in the exponent)
    assert relerr(out2, want2) < 5e-5 and torch.equal(out2, ops.attention_fwd_f32(qkv2.cuda(), B, N, H, scale))


@pytest.mark.parametrize("R,C", [(768, 3072), (1000, 768), (8, 12), (2304, 768)])
@pytest.mark.parametrize("nseg", [3, 6])
def test_weight_split_equals_the_two_split_passes(ops, R, C, nseg):
    """mv_weight_split: the role-1 pieces of an nn.Linear weight for its forward product and of its transpose for the dX product,
    both from one read -- bit-identical to mv_split2/3_bf16(role 1) of w and of a transposed copy; and ops.split_weight hands out
    exactly those (a parameter that takes gradients gets both layouts in one launch)."""
    from myrtle_vision.hip.lib import lib, check
    w = (torch.randn(R, C, generator=g(1)) * 0.3).cuda()
    with ops.segments(nseg):
        want_f = ops.split3(w, R, C, C, 1)
        want_t = ops.split3(w.t().contiguous(), C, R, R, 1)
        fwd = torch.full((R, nseg * C), float("nan"), dtype=torch.bfloat16, device="cuda")
        dx = torch.full((C, nseg * R), float("nan"), dtype=torch.bfloat16, device="cuda")
        check(lib().mv_weight_split(w.data_ptr(), fwd.data_ptr(), dx.data_ptr(), R, C, nseg, torch.cuda.current_stream().cuda_stream),
              "weight_split")
        assert torch.equal(fwd, want_f) and torch.equal(dx, want_t)
        only = torch.full_like(dx, float("nan"))
        check(lib().mv_weight_split(w.data_ptr(), None, only.data_ptr(), R, C, nseg, torch.cuda.current_stream().cuda_stream),
              "weight_split")
        assert torch.equal(only, want_t)
        p = torch.nn.Parameter(w.clone())
        assert torch.equal(ops.split_weight(p, "fwd"), want_f) and torch.equal(ops.split_weight(p, "dx"), want_t)
        with torch.no_grad():
            p.mul_(2.0)                                                   # version bump: both layouts refresh
        assert torch.equal(ops.split_weight(p, "dx").float(), want_t.float() * 2) and torch.equal(ops.split_weight(p, "fwd").float(), want_f.float() * 2)


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (3, 50, 1), (1, 17, 12), (2, 208, 2), (1, 193, 2), (2, 257, 2), (1, 209, 1), (1, 288, 1)])
@pytest.mark.parametrize("gscale", [1.0, 3.0e-7, 4.0e4])
def test_attention_f16_fwd_bwd(ops, B, N, H, gscale):
    """The attention core of precision "bf16x3": the fused bf16 kernels instantiated on IEEE-half operands (fp32 sums, softmax,
    outputs).  Against fp64 on the SAME half-rounded q/k/v: forward to 2^-11-class error (the only roundings left are P -> half
    and the fp32 sums); backward to 2e-3 of each of dq / dk / dv (P, dS and dO in half), and -- the point of the scaling by a power
    of two -- the SAME relative error whether the incoming gradient is O(1), 3e-7 (far below half's normal range, 6e-5) or 4e4
    (above half's largest value divided by the key count)."""
    scale = 64 ** -0.5
    qkv = torch.randn(B, N, 3 * H * 64, generator=g(1)) * 1.2
    dout = torch.randn(B, N, H * 64, generator=g(2)) * gscale
    q16 = ops.cast_f16(qkv.cuda())
    assert q16.dtype == torch.float16 and float((q16.cpu() != qkv.half()).float().mean()) < 2e-4       # (ties: see the GEMM test)
    assert bool(((q16.cpu().float() - qkv).abs() <= qkv.abs() * 2.0 ** -11 + 2.0 ** -24).all())
    ref_in = q16.cpu().double().requires_grad_(True)
    want, _ = attn_ref(ref_in, H, scale)
    want.backward(dout.double())
    out, lse = ops.attention_fwd_f16(q16, B, N, H, scale)
    assert out.dtype == torch.float32 and relerr(out, want) < 6e-4
    q, k, _ = q16.cpu().double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    assert float((lse.cpu().double() - torch.logsumexp((q @ k.transpose(-2, -1)) * scale, dim=-1)).abs().max()) < 2e-5
    dqkv = ops.attention_bwd_f16(q16, out, dout.cuda(), lse, B, N, H, scale)
    assert dqkv.dtype == torch.float32 and bool(torch.isfinite(dqkv).all())
    got, ref = dqkv.cpu().view(B, N, 3, H, 64), ref_in.grad.view(B, N, 3, H, 64)
    for i, name in enumerate("qkv"):
        assert relerr(got[:, :, i], ref[:, :, i]) < 2e-3, (name, relerr(got[:, :, i], ref[:, :, i]))
    # the split-output form (what the bf16x3h block runs): the bf16 pieces of exactly those fp32 values, and per-image column sums
    for nseg in (3, 6):
        with ops.segments(nseg):
            part = torch.empty(B, 3 * H * 64, device="cuda")
            pieces = ops.attention_bwd_f16(q16, out, dout.cuda(), lse, B, N, H, scale, split=True, colsum=part)
            assert torch.equal(pieces, ops.split_ex(dqkv.view(B * N, 3 * H * 64), B * N, 3 * H * 64))
        assert relerr(part, dqkv.double().sum(1)) < 1e-5
    # deterministic, and an all-zero gradient gives exact zeros (scale 1, no 0 * inf)
    assert torch.equal(dqkv, ops.attention_bwd_f16(q16, out, dout.cuda(), lse, B, N, H, scale))
    assert not ops.attention_bwd_f16(q16, out, torch.zeros_like(dout).cuda(), lse, B, N, H, scale).any()


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (1, 257, 2), (3, 50, 1), (1, 17, 12), (2, 208, 2), (1, 272, 1)])
def test_attention_fused_fp32_backward(ops, B, N, H):
    """mv_attention_fwd_f32_lse + mv_attention_bwd_f32 (fp32 training without the [B, H, N, N] tensors) against fp64
    autograd and against the materialised fp32 backward they replace."""
    scale = 64 ** -0.5
    qkv = torch.randn(B, N, 3 * H * 64, generator=g(1)) * 1.5
    dout = torch.randn(B, N, H * 64, generator=g(2))
    ref_in = qkv.double().requires_grad_(True)
    want, _ = attn_ref(ref_in, H, scale)
    want.backward(dout.double())
    out, lse = ops.attention_fwd_f32_lse(qkv.cuda(), B, N, H, scale)
    assert relerr(out, want) < 2e-6 and torch.equal(out, ops.attention_fwd_f32(qkv.cuda(), B, N, H, scale))
    q, k, _ = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    assert float((lse.cpu().double() - torch.logsumexp((q @ k.transpose(-2, -1)) * scale, dim=-1)).abs().max()) < 2e-5
    dqkv = ops.attention_bwd_f32_fused(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale)
    got, ref = dqkv.cpu().view(B, N, 3, H, 64), ref_in.grad.view(B, N, 3, H, 64)
    for i, name in enumerate("qkv"):
        assert relerr(got[:, :, i], ref[:, :, i]) < 5e-6, name
    probs = ops.attention_probs_fp32(qkv.cuda(), B, N, H, 64, scale)
    mat = ops.attention_bwd_fp32(probs, qkv.cuda(), dout.cuda(), B, N, H, 64, scale)
    assert relerr(dqkv, mat.double().cpu()) < 5e-6
    assert torch.equal(dqkv, ops.attention_bwd_f32_fused(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale))   # deterministic


def test_attention_core_dispatch_fp32(ops):
    """attention_core: fp32 input without gradient -> the fused fp32 forward kernel; with gradient -> the fused forward +
    backward pair (no probabilities kept); a hook on attn_output always materialises."""
    from myrtle_vision.hip import functional as F
    qkv = torch.randn(2, 197, 3 * 2 * 64, generator=g(1)).cuda()
    with torch.no_grad():
        a = F.attention_core(qkv, 2, 0.125, None)
    qg = qkv.clone().requires_grad_(True)
    b = F.attention_core(qg, 2, 0.125, None)
    seen = []
    qh = qkv.clone().requires_grad_(True)
    c = F.attention_core(qh, 2, 0.125, lambda p: (seen.append(p.shape), p)[1])
    assert b.requires_grad and not a.requires_grad and seen == [(2, 2, 197, 197)]
    assert torch.equal(a, b.detach()) and relerr(b, c.detach().double().cpu()) < 2e-6
    dout = torch.randn(2, 197, 128, generator=g(2)).cuda()
    b.backward(dout)
    c.backward(dout)
    assert relerr(qg.grad, qh.grad.double().cpu()) < 5e-6          # fused backward == materialised backward


# ---------------------------------------------------------------- elementwise / layout
@pytest.mark.parametrize("B,C,H,W,p", [(3, 3, 224, 224, 16), (2, 3, 256, 256, 16), (2, 1, 32, 48, 8), (1, 3, 30, 30, 6)])
def test_patchify_exact(ops, B, C, H, W, p):
    img = torch.randn(B, C, H, W, generator=g(1))
    want = patchify_oracle(img, p).reshape(-1, p * p * C)
    assert torch.equal(ops.patchify(img.cuda(), p, torch.float32).cpu(), want)
    assert torch.equal(ops.patchify(img.cuda(), p, torch.bfloat16).cpu(), bf(want))


def test_embed_helpers(ops):
    B, T, D = 5, 197, 192
    cls, pos = torch.randn(D, generator=g(1)), torch.randn(T, D, generator=g(2))
    x = torch.zeros(B, T, D, device="cuda")
    ops.embed_cls(cls.cuda(), pos.cuda(), x, B, T, D)
    assert torch.equal(x[:, 0].cpu(), (cls + pos[0]).expand(B, D))
    dx = torch.randn(B, T, D, generator=g(3))
    dpos, dcls = ops.embed_bwd(dx.cuda(), B, T, D)
    assert relerr(dpos, dx.double().sum(0)) < 1e-6 and relerr(dcls, dx[:, 0].double().sum(0)) < 1e-6
    rows = ops.gather_patch_rows(dx.cuda(), B, T, D, torch.bfloat16)
    assert torch.equal(rows.cpu(), bf(dx[:, 1:].reshape(-1, D)))
    # round 4: the two of them in one pass over dx (what _PatchEmbed.backward runs), batch sizes around the 8-row stride
    for B2, T2, D2 in [(5, 197, 192), (256, 197, 768), (3, 257, 192), (1, 2, 4), (9, 17, 132)]:
        dx2 = torch.randn(B2, T2, D2, generator=g(4))
        for dt in (torch.bfloat16, torch.float32):
            dpos2, dcls2, dy2 = ops.embed_bwd_gather(dx2.cuda(), B2, T2, D2, dt)
            want = dx2[:, 1:].reshape(-1, D2)
            assert torch.equal(dy2.cpu(), bf(want) if dt == torch.bfloat16 else want)
            assert relerr(dpos2, dx2.double().sum(0)) < 2e-6 and relerr(dcls2, dx2[:, 0].double().sum(0)) < 2e-6


def test_cast_weightprep_gelu_add(ops):
    x = torch.randn(1000003, generator=g(1))
    assert torch.equal(ops.cast(x.cuda(), torch.bfloat16).cpu(), bf(x))
    assert torch.equal(ops.cast(bf(x).cuda(), torch.float32).cpu(), bf(x).float())
    w = torch.randn(45, 192, generator=g(2))
    pw = ops.prepared_weight(w.cuda())
    assert pw.w.shape == (45, 192) and pw.wt.shape == (192, 48)
    assert torch.equal(pw.w.cpu(), bf(w)) and torch.equal(pw.wt[:, :45].cpu(), bf(w.t())) and (pw.wt[:, 45:] == 0).all()
    h = torch.randn(4099, generator=g(3)) * 2
    assert relerr(ops.gelu_fwd(h.cuda()), gelu_erf(h.double())) < 1e-6
    dy = torch.randn(4099, generator=g(4))
    assert relerr(ops.gelu_bwd(h.cuda(), dy.cuda()), dy.double() * dgelu64(h)) < 2e-6
    assert torch.equal(ops.add_f32(h.cuda(), dy.cuda()).cpu(), h + dy)


def test_weight_prep_batch_refreshes_every_stale_weight_in_one_launch(ops):
    shapes = [(45, 192), (768, 768), (10, 3072), (1000, 71)]          # odd sizes: zero pads on either copy
    ws = [torch.randn(r, c, generator=g(20 + i)).cuda() for i, (r, c) in enumerate(shapes)]
    pws = [ops.prepared_weight(w) for w in ws]                        # first use: one mv_weight_prep each
    for pw in pws:
        pw.w.fill_(7.0)
        pw.wt.fill_(7.0)                                              # poison, pads included
    new = [torch.randn(r, c, generator=g(40 + i)) for i, (r, c) in enumerate(shapes)]
    for w, n in zip(ws, new):
        w.copy_(n)                                                    # in-place update bumps _version -> all stale
    assert ops.prepared_weight(ws[2]) is pws[2]                       # one mv_weight_prep_batch over all four
    for pw, w, n in zip(pws, ws, new):
        assert pw.version == w._version                               # ... so the others are already fresh
        r, c = n.shape
        assert torch.equal(pw.w[:, :c].cpu(), bf(n)) and (pw.w[:, c:] == 0).all()
        assert torch.equal(pw.wt[:, :r].cpu(), bf(n.t())) and (pw.wt[:, r:] == 0).all()
    before = [pw.version for pw in pws]
    assert ops.prepared_weight(ws[0]) is pws[0] and [pw.version for pw in pws] == before      # nothing stale: no work


# ---------------------------------------------------------------- quantisers: bit-exact vs the oracle restatement
def test_quant_float_bit_exact(ops):
    gg = g(7)
    x = torch.randn(300001, generator=gg) * torch.exp(torch.randn(300001, generator=gg) * 5)
    x[:8] = torch.tensor([0.0, -0.0, 65504.0, 65520.0, 1e9, 2.0 ** -24, 2.0 ** -25, -2.0 ** -26])
    for e, m in [(5, 10), (8, 10), (4, 3), (8, 7)]:
        got = ops.quant_float(x.cuda(), e, m).cpu().numpy()
        want = quant_oracle.float_quantize(x.numpy(), e, m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (e, m)


def test_quant_fixed_and_affine_bit_exact(ops):
    x = torch.randn(100001, generator=g(8)) * 3
    for wl, fl in [(11, 9), (11, 8), (11, 7), (8, 4)]:
        got = ops.quant_fixed(x.cuda(), wl, fl).cpu().numpy()
        assert np.array_equal(got, quant_oracle.fixed_point_quantize(x.numpy(), wl, fl)), (wl, fl)
    s, z = quant_oracle.affine_qparams(float(x.min()), float(x.max()), 0, 255, False)
    got = ops.quant_affine(x.cuda(), s, z, 0, 255).cpu().numpy()
    assert np.array_equal(got, quant_oracle.fake_quant_affine(x.numpy(), s, z, 0, 255))
    st = torch.tensor([float("inf"), float("-inf"), 0, 0]).cuda()
    ops.minmax_update(x.cuda(), st)
    ops.minmax_update((x * 0.5 - 20).cuda(), st)
    assert float(st[0]) == float((x * 0.5 - 20).min()) and float(st[1]) == float(x.max())


# ---------------------------------------------------------------- loss / upsample / optimiser
@pytest.mark.parametrize("B,C", [(8, 45), (256, 1000), (3, 17)])
def test_cross_entropy_cls(ops, B, C):
    logits = torch.randn(B, C, generator=g(1)) * 3
    labels = torch.randint(0, C, (B,), generator=g(2))
    ref = logits.double().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(ref, labels)
    l.backward()
    loss, dl, am = ops.cross_entropy(logits.cuda(), labels.cuda(), want_grad=True, want_argmax=True)
    assert abs(float(loss) - float(l)) < 1e-5 * max(1, abs(float(l)))
    assert relerr(dl, ref.grad) < 1e-5
    assert torch.equal(am.cpu(), logits.argmax(1))
    ld = (C + 7) & ~7
    _, dlp, _ = ops.cross_entropy(logits.cuda(), labels.cuda(), want_grad=True, grad_dtype=torch.bfloat16, ld_dl=ld)
    assert dlp.shape == (B, ld) and (dlp[:, C:] == 0).all()
    assert relerr(dlp[:, :C].float(), ref.grad) < 2.0 ** -8


def test_cross_entropy_seg(ops):
    B, C, S = 2, 17, 56
    logits = torch.randn(B, C, S, S, generator=g(1)) * 2
    labels = torch.randint(0, C, (B, S, S), generator=g(2))
    ref = logits.double().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(ref, labels)
    l.backward()
    loss, dl, am = ops.cross_entropy(logits.cuda(), labels.cuda(), want_grad=True, want_argmax=True)
    assert abs(float(loss) - float(l)) < 1e-5 * abs(float(l))
    assert relerr(dl, ref.grad) < 1e-5
    assert torch.equal(am.cpu(), logits.argmax(1))


def test_cross_entropy_ignore_index_and_bad_labels(ops):
    """nn.CrossEntropyLoss() label semantics (classification/train.py:170; DLRSD's PNG-1 can yield -1):
    -100 is skipped and left out of the mean; any other out-of-range label is never dereferenced and poisons the loss."""
    B, C = 16, 45
    logits = torch.randn(B, C, generator=g(1)) * 3
    labels = torch.randint(0, C, (B,), generator=g(2))
    labels[3] = -100
    labels[11] = -100
    ref = logits.double().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(ref, labels)                      # ignore_index = -100, mean over 14
    l.backward()
    loss, dl, _ = ops.cross_entropy(logits.cuda(), labels.cuda(), want_grad=True)
    assert abs(float(loss) - float(l)) < 1e-5 * max(1, abs(float(l)))
    assert relerr(dl, ref.grad) < 1e-5 and float(dl[3].abs().max()) == 0.0 and float(dl[11].abs().max()) == 0.0
    # segmentation layout
    S = 24
    lg = torch.randn(2, 17, S, S, generator=g(3))
    lb = torch.randint(0, 17, (2, S, S), generator=g(4))
    lb[0, :5] = -100
    ref = lg.double().requires_grad_(True)
    l = torch.nn.functional.cross_entropy(ref, lb)
    l.backward()
    loss, dl, _ = ops.cross_entropy(lg.cuda(), lb.cuda(), want_grad=True)
    assert abs(float(loss) - float(l)) < 1e-5 * abs(float(l)) and relerr(dl, ref.grad) < 1e-5
    # out-of-range (not the ignore index): loud NaN loss, zero gradient row, no fault
    for bad in (-1, C, 10 ** 9):
        lab = labels.clone()
        lab[5] = bad
        loss, dl, _ = ops.cross_entropy(logits.cuda(), lab.cuda(), want_grad=True)
        assert torch.isnan(loss).all() and float(dl[5].abs().max()) == 0.0 and torch.isfinite(dl).all()
    # every label ignored: nan, as torch
    loss, _, _ = ops.cross_entropy(logits.cuda(), torch.full((B,), -100).cuda(), want_grad=True)
    assert torch.isnan(loss).all()


def test_seg_ce_fused_tail_ignore_index(ops):
    B, C, g_in, size = 2, 17, 14, 224
    small = torch.randn(B, g_in * g_in, C, generator=g(1)) * 2
    labels = torch.randint(0, C, (B, size, size), generator=g(2))
    labels[0, 10:40, :] = -100
    labels[1, :, 100:120] = -100
    ref = small.double().transpose(1, 2).reshape(B, C, g_in, g_in).requires_grad_(True)
    big = torch.nn.functional.interpolate(ref, size=(size, size), mode="bilinear", align_corners=False)
    l = torch.nn.functional.cross_entropy(big, labels)
    l.backward()
    want_grad = ref.grad.reshape(B, C, -1).transpose(1, 2).reshape(B * g_in * g_in, C)
    sm = small.cuda().view(B * g_in * g_in, C)
    stats, lse, pred, lab = ops.seg_ce_fwd(sm, labels.cuda(), B, C, g_in, g_in, size, size)
    assert abs(float(stats[0]) - float(l)) < 2e-6 * max(1.0, abs(float(l)))
    assert float(stats[2]) == float((labels != -100).sum()) and float(stats[3]) == 0.0
    assert abs(float(stats[1]) - float((big.argmax(1) == labels).double().mean())) < 1e-4      # accuracy over ALL pixels
    ds = ops.seg_ce_bwd(sm, lab, lse, B, C, g_in, g_in, size, size, stats=stats)
    assert relerr(ds, want_grad) < 1e-5
    labels[0, 0, 0] = -1                                                    # DLRSD pixel value 0 -> label -1: loud, not a fault
    stats, lse, pred, lab = ops.seg_ce_fwd(sm, labels.cuda(), B, C, g_in, g_in, size, size)
    assert torch.isnan(stats[0]) and float(stats[3]) == 1.0


@pytest.mark.parametrize("g_in,size", [(14, 224), (16, 256), (7, 20)])
def test_upsample_bilinear(ops, g_in, size):
    B, C = 2, 17
    small = torch.randn(B, g_in * g_in, C, generator=g(1))              # decoder GEMM layout [B, h*w, C]
    ref = small.double().transpose(1, 2).reshape(B, C, g_in, g_in).requires_grad_(True)
    want = torch.nn.functional.interpolate(ref, size=(size, size), mode="bilinear", align_corners=False)
    dbig = torch.randn(B, C, size, size, generator=g(2))
    want.backward(dbig.double())
    big = ops.upsample_bilinear_fwd(small.cuda(), g_in * g_in * C, 1, C, B, C, g_in, g_in, size, size)
    assert relerr(big, want) < 2e-6
    dsmall = torch.empty(B, g_in * g_in, C, device="cuda")
    ops.upsample_bilinear_bwd(dbig.cuda(), dsmall, g_in * g_in * C, 1, C, B, C, g_in, g_in, size, size)
    assert relerr(dsmall, ref.grad.reshape(B, C, -1).transpose(1, 2)) < 5e-6


@pytest.mark.parametrize("B,C,g_in,size", [(3, 17, 14, 224), (2, 5, 4, 50), (1, 32, 16, 256), (2, 17, 7, 20)])
def test_seg_ce_fused_tail(ops, B, C, g_in, size):
    """mv_seg_ce_fwd/bwd == CrossEntropyLoss()(interpolate(small, bilinear), labels) + argmax, without the big logits
    (vit.py:355,371 + segmentation/train.py:188,261-265); also against the unfused HIP composition."""
    small = torch.randn(B, g_in * g_in, C, generator=g(1)) * 2             # decoder GEMM layout [B, h*w, C]
    labels = torch.randint(0, C, (B, size, size), generator=g(2))
    ref = small.double().transpose(1, 2).reshape(B, C, g_in, g_in).requires_grad_(True)
    big = torch.nn.functional.interpolate(ref, size=(size, size), mode="bilinear", align_corners=False)
    l = torch.nn.functional.cross_entropy(big, labels)
    l.backward()
    want_grad = ref.grad.reshape(B, C, -1).transpose(1, 2).reshape(B * g_in * g_in, C)
    assert ops.seg_ce_supported(C, g_in, g_in, size)
    sm = small.cuda().view(B * g_in * g_in, C)
    stats, lse, pred, lab = ops.seg_ce_fwd(sm, labels.cuda(), B, C, g_in, g_in, size, size)
    assert abs(float(stats[0]) - float(l)) < 2e-6 * max(1.0, abs(float(l)))
    want_pred = big.argmax(1)
    # arg-max may differ from the fp64 reference only where the top-2 margin is at fp32 rounding level
    top2 = big.detach().topk(2, dim=1).values
    safe = (top2[:, 0] - top2[:, 1]) > 1e-5
    assert torch.equal(pred.cpu().long()[safe], want_pred[safe])
    assert abs(float(stats[1]) - float((want_pred == labels).double().mean())) < 1e-4
    assert relerr(lse, torch.logsumexp(big.detach(), dim=1)) < 2e-6
    ds = ops.seg_ce_bwd(sm, lab, lse, B, C, g_in, g_in, size, size)
    assert relerr(ds, want_grad) < 1e-5
    # zero-padded bf16 layout read by the decoder's dW / dX GEMMs, and the grad_scale argument
    ld = (C + 7) & ~7
    dsp = ops.seg_ce_bwd(sm, lab, lse, B, C, g_in, g_in, size, size, grad_dtype=torch.bfloat16, ld=ld, grad_scale=2.0)
    assert dsp.shape == (B * g_in * g_in, ld) and (dsp[:, C:] == 0).all()
    assert relerr(dsp[:, :C].float(), 2.0 * want_grad) < 2.0 ** -8
    # unfused HIP composition: same loss, same class map
    bigh = ops.upsample_bilinear_fwd(sm, g_in * g_in * C, 1, C, B, C, g_in, g_in, size, size)
    loss_u, dl_u, am_u = ops.cross_entropy(bigh, labels.cuda(), want_grad=True, want_argmax=True)
    assert abs(float(loss_u) - float(stats[0])) < 2e-6 * max(1.0, abs(float(l)))
    assert (am_u.cpu() != pred.cpu().long()).float().mean() < 1e-4
    # deterministic: a second launch is bit-identical
    ds2 = ops.seg_ce_bwd(sm, lab, lse, B, C, g_in, g_in, size, size)
    assert torch.equal(ds, ds2)


def test_seg_ce_unsupported_shapes_are_rejected(ops):
    assert not ops.seg_ce_supported(33, 14, 14, 224)
    assert not ops.seg_ce_supported(17, 32, 32, 512)
    small = torch.zeros(40 * 40, 17, device="cuda")
    labels = torch.zeros(1, 640, 640, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError):
        ops.seg_ce_fwd(small, labels, 1, 17, 40, 40, 640, 640)          # 40*40*17*4 B > 64 KB of LDS


def test_adamw_matches_torch(ops):
    n = 100003
    p0, gr = torch.randn(n, generator=g(1)), torch.randn(n, generator=g(2))
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    p, m, v = p0.clone().cuda(), torch.zeros(n).cuda(), torch.zeros(n).cuda()
    for step in range(1, 4):
        ref.grad = gr * step
        opt.step()
        ops.adamw_step(p, (gr * step).cuda(), m, v, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.05, step=step)
    assert relerr(p, ref.data) < 2e-6


@pytest.mark.parametrize("M,N,K", [(394, 768, 768), (50, 45, 200), (1030, 300, 3072)])
def test_int8_codes_gemm_equals_fake_quant_linear(ops, M, N, K):
    """Converted-int8 Linear on the MFMA path: integer codes (exact in bf16) x integer codes, fp32 accumulation, scale in the
    epilogue == linear(fake_quantize(x), fake_quantize(W)) + b as torch computes it in fp32."""
    x = torch.randn(M, K, generator=g(1)) * 2 + 0.3
    w = torch.randn(N, K, generator=g(2)) * K ** -0.5
    b = torch.randn(N, generator=g(3))
    s_x = float((x.max() - min(x.min(), 0)) / 255.0)
    z_x = int(min(max(round(-float(min(x.min(), 0)) / s_x), 0), 255))
    s_w = float(w.abs().max() / 127.5)
    xq = torch.fake_quantize_per_tensor_affine(x, s_x, z_x, 0, 255)
    wq = torch.fake_quantize_per_tensor_affine(w, s_w, 0, -128, 127)
    want = torch.nn.functional.linear(xq.double(), wq.double(), b.double())
    xc = ops.quant_affine_codes(x.cuda(), M, K, s_x, z_x, 0, 255)
    # the GELU pre-op is the unfused (exact-erf) gelu followed by the same quantiser up to the pre-op's 1.5e-7-accurate erf:
    # a code may move by one where the exact value sits within 1.5e-7 of a rounding boundary (about 1 element in 10^5)
    fused_codes = ops.quant_affine_codes(x.cuda(), M, K, s_x, z_x, 0, 255, pre_gelu=True).float()
    plain_codes = ops.quant_affine_codes(ops.gelu_fwd(x.cuda()), M, K, s_x, z_x, 0, 255).float()
    assert float((fused_codes - plain_codes).abs().max()) <= 1.0 and float((fused_codes != plain_codes).float().mean()) < 2e-4
    assert xc.shape == (M, (K + 7) & ~7) and xc.dtype == torch.bfloat16
    codes = xc[:, :K].float().cpu()
    assert torch.equal(codes, torch.round(xq / s_x))                     # the integer (q - z), exactly
    assert (xc[:, K:] == 0).all() and codes.abs().max() <= 255
    wc = torch.zeros(N, (K + 7) & ~7, dtype=torch.bfloat16)
    wc[:, :K] = torch.round(wq / s_w)
    out = torch.empty(M, N, device="cuda")
    ops.linear_codes(xc, wc.cuda(), M, N, K, s_x * s_w, b.cuda(), out)
    assert relerr(out, want) < 2e-6


@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (197 * 8, 3072, 768), (1000, 768, 3072), (300, 512, 256)])
def test_int8_mfma_gemm_is_the_exact_integer_product(ops, M, N, K):
    """mv_gemm_nt_i8 (v_mfma_i32_16x16x64_i8): int32 accumulation is the exact integer dot product; with A8 = q - 128 and
    icorr[n] = (128 - z) sum_k w[n][k] the result equals the integer-codes product on the bf16 MFMA (bit for bit after the
    same scale/bias epilogue) and torch's linear(fake_quantize(x), fake_quantize(W)) + b."""
    x = torch.randn(M, K, generator=g(1)) * 2 + 0.3
    w = torch.randn(N, K, generator=g(2)) * K ** -0.5
    b = torch.randn(N, generator=g(3))
    s_x = float((x.max() - min(x.min(), 0)) / 255.0)
    z_x = int(min(max(round(-float(min(x.min(), 0)) / s_x), 0), 255))
    s_w = float(w.abs().max() / 127.5)
    xq = torch.fake_quantize_per_tensor_affine(x, s_x, z_x, 0, 255)
    wq = torch.fake_quantize_per_tensor_affine(w, s_w, 0, -128, 127)
    want = torch.nn.functional.linear(xq.double(), wq.double(), b.double())
    x8 = ops.quant_affine_i8(x.cuda(), M, K, s_x, z_x)
    assert x8.dtype == torch.int8 and x8.shape == (M, (K + 15) & ~15)
    q = torch.round(xq / s_x) + z_x                                        # the uint8 level
    assert torch.equal(x8[:, :K].cpu().to(torch.int64), (q - 128).to(torch.int64))
    wcodes = torch.round(wq / s_w)
    w8 = torch.zeros(N, (K + 15) & ~15, dtype=torch.int8)
    w8[:, :K] = wcodes.to(torch.int8)
    icorr = ((128 - z_x) * wcodes.sum(1).to(torch.int64)).to(torch.int32)
    out = torch.empty(M, N, device="cuda")
    ops.linear_i8(x8, w8.cuda(), M, N, K, s_x * s_w, b.cuda(), icorr.cuda(), out)
    # exact integer reference: (q - z) . w in int64, then the fp32 epilogue fmaf(acc, alpha, bias)
    acc = (q - z_x).to(torch.int64) @ wcodes.to(torch.int64).t()
    assert acc.abs().max() < 2 ** 24                                       # so the float conversion is exact
    ref32 = torch.addcmul(b, acc.float(), torch.tensor(s_x * s_w, dtype=torch.float32))   # one rounding, like fmaf? (checked loosely)
    assert relerr(out, want) < 2e-6 and relerr(out, ref32.double()) < 1e-6
    # against the round-1 path (integer codes on the bf16 MFMA): identical bits
    xc = ops.quant_affine_codes(x.cuda(), M, K, s_x, z_x, 0, 255)
    wc = torch.zeros(N, (K + 7) & ~7, dtype=torch.bfloat16)
    wc[:, :K] = wcodes
    out_codes = torch.empty(M, N, device="cuda")
    ops.linear_codes(xc, wc.cuda(), M, N, K, s_x * s_w, b.cuda(), out_codes)
    assert torch.equal(out, out_codes)
    # fused residual and bf16 output
    res = torch.randn(M, N, generator=g(4)).cuda()
    out_r, out_rc = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    ops.linear_i8(x8, w8.cuda(), M, N, K, s_x * s_w, b.cuda(), icorr.cuda(), out_r, residual=res)
    ops.linear_codes(xc, wc.cuda(), M, N, K, s_x * s_w, b.cuda(), out_rc, residual=res)
    assert torch.equal(out_r, out_rc)
    out_b = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    ops.linear_i8(x8, w8.cuda(), M, N, K, s_x * s_w, b.cuda(), icorr.cuda(), out_b)
    assert torch.equal(out_b, out.bfloat16())
    # the GELU pre-op of the int8 quantiser == unfused (exact-erf) gelu then quantise, up to the fast erf's rare one-code moves
    fused8 = ops.quant_affine_i8(x.cuda(), M, K, s_x, z_x, pre_gelu=True).float()
    plain8 = ops.quant_affine_i8(ops.gelu_fwd(x.cuda()), M, K, s_x, z_x).float()
    assert float((fused8 - plain8).abs().max()) <= 1.0 and float((fused8 != plain8).float().mean()) < 2e-4


def test_int8_vit_base_dim_matches_torch_fake_quant():
    """BASELINE config 5 at ViT-B/16 width (dim 768, 12 heads, mlp 3072; depth 2 keeps it short): the converted model on the
    int8 MFMA == the same model with every Int8Linear replaced by torch's own fake-quant arithmetic
    linear(fake_quantize_per_tensor_affine(x), fake_quantize(W)) + b (what its grad-mode path computes through the fp32
    kernels), == the integer-codes path on the bf16 MFMA bit for bit."""
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.quantize import Int8Linear
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(3)
    vit = ViT(precision="bf16", q_format="PyTorchINT8", decoder="classification", image_size=224, patch_size=16, num_classes=1000,
              dim=768, depth=2, heads=12, mlp_dim=3072, dropout=0.0, emb_dropout=0.0).cuda()
    gen = torch.Generator().manual_seed(4)
    vit.train()
    with torch.no_grad():
        for _ in range(2):
            vit(torch.randn(8, 3, 224, 224, generator=gen).cuda())
    vit.convert()
    vit.eval()
    img = torch.randn(8, 3, 224, 224, generator=gen).cuda()
    used = []
    orig = Int8Linear.forward
    with torch.no_grad():
        fast = vit(img)                                                    # int8 MFMA where the shape allows
        Int8Linear.use_i8 = False
        try:
            codes = vit(img)                                               # integer codes on the bf16 MFMA (round 1)
        finally:
            Int8Linear.use_i8 = True
    assert torch.equal(fast, codes)
    # torch's own fake-quant arithmetic on the CPU for one layer of that model, at its calibrated parameters
    lin = vit.transformer.layers[0][1].fn.fn.net[0][1]
    assert isinstance(lin, Int8Linear) and lin.weight_i8 is not None
    s_x, z_x = lin.act_observer.frozen
    x = torch.randn(197 * 4, 768, generator=gen)
    want = torch.nn.functional.linear(torch.fake_quantize_per_tensor_affine(x, s_x, z_x, 0, 255).double(),
                                      lin.weight.detach().double().cpu(), lin.bias.detach().double().cpu())
    with torch.no_grad():
        got = lin(x.cuda())
    assert relerr(got, want) < 2e-6
    # grad mode: fp32 fake-quant (straight-through) kernels end to end.  Same arithmetic up to fp32 summation order, but 8-bit
    # quantisers are discontinuous: an ulp of difference in front of one flips a code (0.4 % of the tensor's range), and at
    # this width a few of the 3 M activations per layer do (measured 5e-3 of the logits' range)
    slow = vit(img)
    assert relerr(fast, slow.detach().double().cpu()) < 2e-2


@pytest.mark.parametrize("M,N,K", [(512, 768, 768), (1576, 3072, 768), (1000, 768, 3072)])
def test_f16_mfma_gemm_of_quantised_operands(ops, M, N, K):
    """mv_quant_float_f16 + mv_gemm_nt_f16: float_quantize(5, 10) values are exact IEEE halves, so the f16 MFMA with fp32
    accumulation gives the fp32 product of the quantised operands (what the reference's nn.qat.Linear computes)."""
    from oracle import quant_oracle
    x = torch.randn(M, K, generator=g(1)) * 3
    w = torch.randn(N, K, generator=g(2)) * K ** -0.5
    b = torch.randn(N, generator=g(3))
    x[0, :8] = torch.tensor([1e-7, -3e-6, 6.1e-5, 7e4, -1e5, 0.0, 65504.0, 2.0 ** -24])      # subnormals, saturation
    xq = torch.from_numpy(quant_oracle.float_quantize(x.numpy(), 5, 10))
    wq = torch.from_numpy(quant_oracle.float_quantize(w.numpy(), 5, 10))
    x16, w16 = ops.quant_float_f16(x.cuda()), ops.quant_float_f16(w.cuda())
    assert x16.dtype == torch.float16 and torch.equal(x16.float().cpu(), xq) and torch.equal(w16.float().cpu(), wq)
    assert torch.equal(ops.quant_float_f16(xq.cuda()), x16)                                   # idempotent
    out = torch.empty(M, N, device="cuda")
    ops.linear_f16(x16, w16, M, N, K, b.cuda(), out)
    assert relerr(out, xq.double() @ wq.double().t() + b.double()) < 2e-6
    res = torch.randn(M, N, generator=g(4)).cuda()
    out2 = torch.empty(M, N, device="cuda")
    ops.linear_f16(x16, w16, M, N, K, b.cuda(), out2, residual=res)
    assert relerr(out2, xq.double() @ wq.double().t() + b.double() + res.double().cpu()) < 2e-6


def test_fp16_qat_model_f16_forward_equals_fp32_path():
    """FP16_32-prepared ViT at ViT-B width: forward products on the f16 matrix cores == the fp32-GEMM path on the same
    quantised values (fp32 summation order apart; quantisers downstream are discontinuous, hence 3e-3 as for the goldens),
    same gradients through the straight-through estimator."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.quantize import QATLinear
    from myrtle_vision.utils.utils import seed_everything
    kw = dict(decoder="classification", image_size=224, patch_size=16, num_classes=1000, dim=768, depth=2, heads=12, mlp_dim=3072)
    gen = torch.Generator().manual_seed(4)
    img, labels = torch.randn(4, 3, 224, 224, generator=gen).cuda(), torch.randint(0, 1000, (4,), generator=gen).cuda()
    res = {}
    for use in (True, False):
        seed_everything(3)
        vit = ViT(q_format="FP16_32", **kw).cuda()
        QATLinear.use_f16 = use
        try:
            logits = vit(img)
            cross_entropy(logits, labels).backward()
        finally:
            QATLinear.use_f16 = True
        res[use] = (logits.detach().double().cpu(), {n: p.grad.double().cpu() for n, p in vit.named_parameters() if p.grad is not None})
    assert relerr(res[True][0], res[False][0]) < 3e-3
    for n, gr in res[False][1].items():
        assert float((res[True][1][n] - gr).norm() / gr.norm().clamp_min(1e-30)) < 2e-2, n
    # and the f16 path is actually taken at this width
    from myrtle_vision.hip import ops as _ops
    seen, orig = [], _ops.linear_f16
    _ops.linear_f16 = lambda *a, **k: (seen.append(a[2:5]), orig(*a, **k))[1]
    try:
        seed_everything(3)
        vit = ViT(q_format="FP16_32", **kw).cuda()
        with torch.no_grad():
            vit(img)
    finally:
        _ops.linear_f16 = orig
    assert len(seen) == 1 + 4 * 2                    # patch embedding + (qkv, proj, fc1, fc2) x 2 blocks; the head has M = 4


def test_split3_ex_fuses_gelu_and_column_sums(ops):
    """mv_split3_bf16_ex: op 0 == the plain split bit for bit; ops 1 / 2 reconstruct gelu(x) / x * gelu'(h) of the standalone
    kernels to an ulp; the column sums are the bias gradient."""
    rows, cols = 1024 + 32, 768
    x, h = torch.randn(rows, cols, generator=g(1)).cuda(), torch.randn(rows, cols, generator=g(2)).cuda()
    cs = torch.empty(cols, device="cuda")
    assert torch.equal(ops.split_ex(x, rows, cols, colsum_out=cs), ops.split3(x, rows, cols, cols, 0))
    assert relerr(cs, x.double().sum(0)) < 2e-6

    def value(s6):                                   # p0 + p1 + p2 (segments 0, 2, 5), and the duplicated segments agree
        v = s6.view(rows, 6, cols).double()
        assert torch.equal(v[:, 0], v[:, 1]) and torch.equal(v[:, 0], v[:, 3]) and torch.equal(v[:, 2], v[:, 4])
        return v[:, 0] + v[:, 2] + v[:, 5]

    # the GELU inside the split kernel may contract its multiplies differently from the standalone kernel: 1 ulp
    a = ops.gelu_fwd(x).double()
    assert ((value(ops.split_ex(x, rows, cols, op=1)) - a).abs() <= a.abs() * 2.0 ** -22 + 1e-30).all()
    dh = ops.gelu_bwd(h, x).double()
    assert ((value(ops.split_ex(x, rows, cols, op=2, h=h, colsum_out=cs)) - dh).abs() <= dh.abs() * 2.0 ** -22 + 1e-30).all()
    assert relerr(cs, dh.sum(0)) < 2e-6


def test_fp32_blocks_on_bf16x6_match_the_fmaf_chain_path():
    """fp32-mode ViT at batch 32 (M = 6304 = 32 x 197 rows: the transformer blocks take the bf16x6 route that keeps operand
    splits instead of activations): logits and every gradient against the same model on mv_gemm_f32 (k-ordered fmaf chain)."""
    from myrtle_vision.hip import ops as _ops
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    kw = dict(decoder="classification", image_size=224, patch_size=16, num_classes=45, dim=192, depth=3, heads=3, mlp_dim=768)
    gen = torch.Generator().manual_seed(5)
    img, labels = torch.randn(32, 3, 224, 224, generator=gen).cuda(), torch.randint(0, 45, (32,), generator=gen).cuda()
    res, taken = {}, []
    orig = _ops.tn_x6
    _ops.tn_x6 = lambda *a, **k: (taken.append(1), orig(*a, **k))[1]
    try:
        for mode in ("bf16x6", "mfma"):
            prev = _ops.set_f32_gemm(mode)
            try:
                seed_everything(3)
                vit = ViT(precision="fp32", **kw).cuda()
                logits = vit(img)
                cross_entropy(logits, labels).backward()
            finally:
                _ops.set_f32_gemm(prev)
            res[mode] = (logits.detach().double().cpu(), {n: p.grad.double().cpu() for n, p in vit.named_parameters() if p.grad is not None})
    finally:
        _ops.tn_x6 = orig
    assert len(taken) == 4 * 3                       # (qkv, proj, fc1, fc2) dW x 3 blocks went through the split-keeping path
    assert relerr(res["bf16x6"][0], res["mfma"][0]) < 2e-5
    assert torch.equal(res["bf16x6"][0].argmax(1), res["mfma"][0].argmax(1))
    assert set(res["bf16x6"][1]) == set(res["mfma"][1])
    for n, gr in res["mfma"][1].items():
        assert float((res["bf16x6"][1][n] - gr).norm() / gr.norm().clamp_min(1e-30)) < 2e-5, n


def test_fused_quantiser_producers_are_bit_identical(ops):
    """LayerNorm / exact-fp32 attention / int8-GEMM+GELU with the NEXT layer's quint8 quantiser fused in produce the same
    int8 codes as producer + mv_quant_affine_i8 (one shared device function, same expressions)."""
    M, D, H = 1024, 768, 12
    x = (torch.randn(M, D, generator=g(1)) * 2 + 0.5).cuda()
    gam, bet = (1 + 0.1 * torch.randn(D, generator=g(2))).cuda(), (0.1 * torch.randn(D, generator=g(3))).cuda()
    s, z = 0.0123, 117
    y, _, _ = ops.layernorm_fwd(x, D, M, D, gam, bet, torch.float32)
    assert torch.equal(ops.layernorm_q8(x, D, M, D, gam, bet, 1e-5, s, z), ops.quant_affine_i8(y, M, D, s, z))
    B, N = 4, 197
    qkv = (torch.randn(B, N, 3 * H * 64, generator=g(4)) * 1.5).cuda()
    o = ops.attention_fwd_f32(qkv, B, N, H, 0.125)
    s2, z2 = 0.004, 131
    assert torch.equal(ops.attention_fwd_f32_q8(qkv, B, N, H, 0.125, s2, z2).view(B * N, H * 64),
                       ops.quant_affine_i8(o.view(B * N, H * 64), B * N, H * 64, s2, z2))
    # int8 GEMM -> GELU -> next quantiser
    Mg, Ng, K = 1024, 3072, 768
    x8 = torch.randint(-128, 128, (Mg, K), generator=g(5), dtype=torch.int8).cuda()
    w8 = torch.randint(-127, 128, (Ng, K), generator=g(6), dtype=torch.int8).cuda()
    bias, icorr = torch.randn(Ng, generator=g(7)).cuda(), torch.randint(-5000, 5000, (Ng,), generator=g(8), dtype=torch.int32).cuda()
    alpha = 3.1e-4
    h = torch.empty(Mg, Ng, device="cuda")
    ops.linear_i8(x8, w8, Mg, Ng, K, alpha, bias, icorr, h)
    s3, z3 = 0.02, 9
    h8 = torch.empty(Mg, Ng, dtype=torch.int8, device="cuda")
    ops.linear_i8(x8, w8, Mg, Ng, K, alpha, bias, icorr, h8, gelu_q8=(s3, z3))
    assert torch.equal(h8, ops.quant_affine_i8(h, Mg, Ng, s3, z3, pre_gelu=True))


def test_int8_blocks_with_fused_quantisers_equal_module_path():
    """Converted PyTorchINT8 ViT at ViT-B width, batch 256 (M = 50 432 = 197 x 256 rows): with every quantiser fused into its
    producer (LayerNorm -> int8, attention -> int8, fc1 epilogue GELU -> int8) the logits are bit-identical to the path that
    writes fp32 activations and quantises them in separate kernels."""
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.quantize import Int8Linear
    from myrtle_vision.utils.utils import seed_everything
    from myrtle_vision.hip import ops as _ops
    seed_everything(3)
    vit = ViT(precision="bf16", q_format="PyTorchINT8", decoder="classification", image_size=224, patch_size=16, num_classes=1000,
              dim=768, depth=2, heads=12, mlp_dim=3072, dropout=0.0, emb_dropout=0.0).cuda()
    gen = torch.Generator().manual_seed(4)
    vit.train()
    with torch.no_grad():
        vit(torch.randn(8, 3, 224, 224, generator=gen).cuda())
    vit.convert()
    vit.eval()
    img = torch.randn(256, 3, 224, 224, generator=gen).cuda()
    seen, orig = [], _ops.layernorm_q8
    _ops.layernorm_q8 = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            fused = vit(img)
            assert len(seen) == 4                        # two blocks x (attention, MLP)
            Int8Linear.fuse_quant = False
            try:
                plain = vit(img)
            finally:
                Int8Linear.fuse_quant = True
            assert len(seen) == 4
    finally:
        _ops.layernorm_q8 = orig
    assert torch.equal(fused, plain)


def test_int8_converted_model_fast_path_equals_fake_quant_path():
    """ViT.convert() for PyTorchINT8 installs Int8Linear: under no_grad it runs integer codes through the MFMA GEMM; with
    grad enabled it runs the fp32 fake-quant (straight-through) path.  Same numbers up to fp32 summation order."""
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.quantize import Int8Linear
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(3)
    vit = ViT(precision="bf16", q_format="PyTorchINT8", decoder="classification", image_size=224, patch_size=16, num_classes=10,
              dim=128, depth=2, heads=2, mlp_dim=256, dropout=0.0, emb_dropout=0.0).cuda()
    gen = torch.Generator().manual_seed(4)
    vit.train()
    with torch.no_grad():
        for _ in range(3):                                                # min/max calibration (test_quantize.py:26-34)
            vit(torch.randn(4, 3, 224, 224, generator=gen).cuda())
    vit.convert()
    vit.eval()
    assert sum(isinstance(m, Int8Linear) for m in vit.modules()) == 2 * 4 + 2      # 4 per block + patch embedding + head
    img = torch.randn(4, 3, 224, 224, generator=gen).cuda()
    with torch.no_grad():
        fast = vit(img)
    from myrtle_vision.hip import ops as _ops0
    prev = _ops0.set_f32_gemm("mfma")
    try:
        slow = vit(img)                                                   # grad mode: fake-quant fp32 path (fmaf-chain GEMMs)
    finally:
        _ops0.set_f32_gemm(prev)
    assert slow.requires_grad and not fast.requires_grad
    assert relerr(fast, slow.detach().double().cpu()) < 1e-4
    assert torch.equal(fast.argmax(1), slow.argmax(1))
    # the default fp32 products (bf16x6) round differently (5e-7): a quantiser downstream may land on the other side of a
    # code boundary, and one flipped code in the class-token row moves a logit by ~1e-3
    slow6 = vit(img)
    assert relerr(fast, slow6.detach().double().cpu()) < 5e-3 and torch.equal(fast.argmax(1), slow6.argmax(1))
    # FeedForward folds nn.GELU into fc2's input quantiser: taken (2 blocks), and bit-identical to the unfolded path
    from myrtle_vision.hip import ops as _ops
    from myrtle_vision.models.vit import GELU
    seen, orig = [], _ops.quant_affine_codes
    _ops.quant_affine_codes = lambda *a, **k: (seen.append(k.get("pre_gelu", False)), orig(*a, **k))[1]
    try:
        with torch.no_grad():
            assert torch.equal(vit(img), fast) and sum(seen) == 2
        # hooks on GELU and on the attention output Dropout switch every int8 block fusion off (GELU fold, residual in the
        # GEMM epilogue, direct to_qkv -> attention -> to_out chaining): the module-by-module path gives the same bits
        from myrtle_vision.models.vit import Attention as _Att
        hooks = [m.register_forward_hook(lambda mod, i, o: None) for m in vit.modules() if isinstance(m, GELU)]
        hooks += [m.to_out[1].register_forward_hook(lambda mod, i, o: None) for m in vit.modules() if isinstance(m, _Att)]
        assert all(m.int8_pair() is None for m in vit.modules() if isinstance(m, _Att))
        seen.clear()
        with torch.no_grad():
            unfolded = vit(img)
        assert sum(seen) == 0 and torch.equal(unfolded, fast)
        for h in hooks:
            h.remove()
    finally:
        _ops.quant_affine_codes = orig
    # opt-in: attention core on the fused bf16 kernel (ViT.convert(bf16_attention=True)); bf16-mode envelope
    from myrtle_vision.models.vit import Attention
    for m in vit.modules():
        if isinstance(m, Attention):
            m.bf16_core = True
    with torch.no_grad():
        approx = vit(img)
    assert approx.dtype == torch.float32 and 0 < relerr(approx, fast.double().cpu()) < 3e-2
    # ... and its fused chaining (bf16 to_qkv output, bf16-input quantiser) equals the cast-based module path bit for bit
    hooks = [m.to_out[1].register_forward_hook(lambda mod, i, o: None) for m in vit.modules() if isinstance(m, Attention)]
    with torch.no_grad():
        assert torch.equal(vit(img), approx)
    for h in hooks:
        h.remove()
