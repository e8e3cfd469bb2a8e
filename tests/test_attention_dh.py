"""GPU: the fused bf16 attention core for 32- and 128-wide heads (mv_attention_fwd_dh / _bwd_dh), any N up to 8 192.

The kernels against fp64 from the same bf16 inputs at the bars tests/test_attention_long.py applies to the 64-wide key-tiled
kernels (same rounding points: P and dS rounded to bf16, fp32 accumulation, outputs rounded once), determinism, the rejections
of the C entry points, the absence of any [B, H, N, N] tensor, and whole models of both widths against the CPU oracle at the
bf16 envelope and against the materialised path (``ops.ATTN_LONG`` off: what these widths took before)."""
import pytest
import torch

from oracle.detinit import det_images, det_labels, det_param
from oracle.vit_oracle import ViTConfig, loss_and_grads

pytestmark = pytest.mark.gpu

WIDTHS = [32, 128]


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
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def attn_ref(qkv, H, dh):
    B, N, _ = qkv.shape
    q, k, v = qkv.double().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * dh), torch.logsumexp(s, dim=-1)


def make(B, N, H, dh, qk_mult=1.0, seed=1):
    qkv = torch.randn(B, N, 3, H, dh, generator=g(seed)) * 1.5
    qkv[:, :, :2] *= qk_mult
    return (qkv.view(B, N, 3 * H * dh).to(torch.bfloat16),
            torch.randn(B, N, H * dh, generator=g(seed + 1)).to(torch.bfloat16))


def check_against_fp64(ops, qkv, dout, B, N, H, dh):
    scale = dh ** -0.5
    ref_in = qkv.double().requires_grad_(True)
    want, lse_ref = attn_ref(ref_in, H, dh)
    want.backward(dout.double())
    out, lse = ops.attention_fwd_dh(qkv.cuda(), B, N, H, dh, scale)
    part = torch.full((B, 3 * H * dh), float("nan"), device="cuda")
    dqkv = ops.attention_bwd_dh(qkv.cuda(), out, dout.cuda(), lse, B, N, H, dh, scale, colsum=part)
    got, ref = dqkv.float().cpu().view(B, N, 3, H, dh), ref_in.grad.view(B, N, 3, H, dh)
    e_out = relerr(out.float(), want)
    e_lse = float((lse.cpu().double() - lse_ref.detach()).abs().max())
    e_g = [relerr(got[:, :, i], ref[:, :, i]) for i in range(3)]
    e_cs = relerr(part.cpu(), dqkv.float().sum(1).cpu())
    e_cs64 = relerr(part.cpu().double(), ref_in.grad.sum(1))
    print(f"dh={dh} B={B} N={N} H={H}: out {e_out:.3e} lse {e_lse:.3e} dq {e_g[0]:.3e} dk {e_g[1]:.3e} dv {e_g[2]:.3e} "
          f"colsum {e_cs:.3e} colsum_vs_fp64 {e_cs64:.3e}")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    # P is rounded to bf16 before P.V (2^-9 per element, averaged over keys) and the output once more
    assert e_out < 1.5e-2
    assert e_lse < 1e-4
    for i, (e, name) in enumerate(zip(e_g, "qkv")):
        if float(ref[:, :, i].abs().max()) == 0.0:
            # N = 1: p = 1, so dS = p (dP - delta) and with it dq and dk are exactly 0 and a relative error does not exist.  dP and
            # delta are two fp32 sums of the same dh products dO_d v_d in different orders: each is within dh 2^-24 sum |dO_d v_d|
            # of the exact value, so |dS| <= 2 dh 2^-24 sum |dO_d v_d| scale, and |dq|, |dk| <= |dS| max(|k|, |q|) (one bf16
            # rounding of dS and one of the result: a factor (1 + 2^-8)^2)
            x = qkv.float().view(B, N, 3, H, dh)
            terms = (dout.float().view(B, N, H, dh).abs() * x[:, :, 2].abs()).sum(-1).max()
            bound = float(2 * dh * 2.0 ** -24 * terms * scale * x[:, :, :2].abs().max() * (1 + 2.0 ** -8) ** 2)
            print(f"  d{name}: exact value 0, largest |got| {float(got[:, :, i].abs().max()):.3e}, bound {bound:.3e}")
            assert float(got[:, :, i].abs().max()) <= bound, name
        else:
            assert e < 3e-2, name
    assert e_cs < 5e-3
    assert e_cs64 < 3e-2
    dq2 = ops.attention_bwd_dh(qkv.cuda(), out, dout.cuda(), lse, B, N, H, dh, scale)          # colsum is optional
    assert torch.equal(dq2, dqkv)


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("dh", WIDTHS)
@pytest.mark.parametrize("B,N,H", [(2, 1, 2), (3, 15, 2), (2, 64, 3), (2, 65, 2), (2, 197, 3), (1, 257, 2), (2, 577, 2),
                                   (1, 1025, 2), (1, 4097, 1)])
def test_dh_attention_vs_fp64(ops, B, N, H, dh):
    qkv, dout = make(B, N, H, dh, seed=3 + N)
    check_against_fp64(ops, qkv, dout, B, N, H, dh)


@pytest.mark.parametrize("dh", WIDTHS)
def test_dh_attention_vs_fp64_with_moving_maxima(ops, dh):
    """q and k four times larger: scores 16x larger, so the running maximum of a query row really moves between key blocks and
    the accumulators are rescaled."""
    qkv, dout = make(1, 577, 2, dh, qk_mult=4.0, seed=23)
    check_against_fp64(ops, qkv, dout, 1, 577, 2, dh)


@pytest.mark.parametrize("dh", WIDTHS)
def test_dh_attention_is_deterministic(ops, dh):
    B, N, H = 2, 1025, 3
    qkv, dout = make(B, N, H, dh, seed=11)
    qkv, dout = qkv.cuda(), dout.cuda()
    runs = []
    for _ in range(2):
        out, lse = ops.attention_fwd_dh(qkv, B, N, H, dh, dh ** -0.5)
        part = torch.empty(B, 3 * H * dh, device="cuda")
        dqkv = ops.attention_bwd_dh(qkv, out, dout, lse, B, N, H, dh, dh ** -0.5, colsum=part)
        runs.append((out, lse, dqkv, part))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def test_dh_entry_points_reject_without_launching(ops):
    """Width 48, N = 0, N = 8 193 and a misaligned pointer come back as error codes; the output buffers keep their contents."""
    from myrtle_vision.hip.lib import lib
    B, N, H = 1, 64, 2
    stream = torch.cuda.current_stream().cuda_stream
    qkv = torch.zeros(B * 8193 * 3 * H * 128, dtype=torch.bfloat16, device="cuda")
    out = torch.full((B * 8193 * H * 128,), 7.0, dtype=torch.bfloat16, device="cuda")
    dqkv = torch.full_like(qkv, 7.0)
    lse = torch.full((B * H * 8193,), 7.0, device="cuda")
    delta = torch.full_like(lse, 7.0)
    p = lambda t: t.data_ptr()
    fwd, bwd = lib().mv_attention_fwd_dh, lib().mv_attention_bwd_dh
    MV_ERR_SHAPE, MV_ERR_ALIGN, MV_ERR_UNSUPPORTED = -1, -2, -4
    for dh, n, code in [(48, N, MV_ERR_UNSUPPORTED), (64, N, MV_ERR_UNSUPPORTED), (32, 0, MV_ERR_SHAPE), (128, 0, MV_ERR_SHAPE),
                        (32, 8193, MV_ERR_SHAPE), (128, 8193, MV_ERR_SHAPE)]:
        assert fwd(p(qkv), p(out), p(lse), B, n, H, dh, 0.125, stream) == code, (dh, n)
        assert bwd(p(qkv), p(out), p(out), p(lse), p(delta), p(dqkv), None, B, n, H, dh, 0.125, stream) == code, (dh, n)
    assert fwd(p(qkv) + 2, p(out), p(lse), B, N, H, 32, 0.125, stream) == MV_ERR_ALIGN
    assert bwd(p(qkv), p(out), p(out), p(lse), p(delta), p(dqkv) + 2, None, B, N, H, 128, 0.125, stream) == MV_ERR_ALIGN
    torch.cuda.synchronize()
    for t in (out, dqkv, lse, delta):
        assert bool((t == 7.0).all())
    with pytest.raises(RuntimeError):
        ops.attention_fwd_dh(qkv[:B * N * 3 * H * 48].view(B, N, 3 * H * 48), B, N, H, 48, 48 ** -0.5)


@pytest.mark.parametrize("dh", WIDTHS)
def test_attention_core_keeps_no_n_squared_tensor(ops, dh):
    from myrtle_vision.hip import functional as F
    B, H, N = 8, 26, 577
    assert B * H * N * N * 4 >= 256 * 2 ** 20
    qkv, dout = make(B, N, H, dh, seed=17)
    qkv = qkv.cuda().requires_grad_(True)
    dout = dout.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = F.attention_core(qkv, H, dh ** -0.5)
    out.backward(dout)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert qkv.grad is not None and bool(torch.isfinite(qkv.grad.float()).all())
    quarter = B * H * N * N * 4 / 4
    # the results the call has to leave behind (out and qkv.grad: 8 dh bytes per (image, head, token)) are not what this test is
    # about, and at dh = 128 they alone are larger than the bar (1 024 > N = 577 bytes): everything else must stay below it
    results = out.numel() * out.element_size() + qkv.grad.numel() * qkv.grad.element_size()
    print(f"dh={dh}: peak growth {grew} B, of which results {results} B; a quarter of [B, H, N, N] fp32 = {quarter:.0f} B")
    assert grew - results < quarter, (grew, results)
    if 8 * dh < N:
        assert grew < quarter, grew          # test_attention_long.py's form, where the results fit under the bar


# ---------------------------------------------------------------- models
MODELS = {32: dict(dim=192, heads=6, dim_head=32, depth=2, mlp_dim=768),           # the golden fixtures' micro widths
          128: dict(dim=384, heads=3, dim_head=128, depth=2, mlp_dim=1536)}        # ViT-Small's widths


def _run_model(ops, kw, params, img, labels, monkeypatch, fused):
    """One forward + backward of the bf16 model -> (logits, gradients, calls of the dh kernels' wrappers)."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    calls = {"fwd": 0, "bwd": 0}
    fwd0, bwd0 = ops.attention_fwd_dh, ops.attention_bwd_dh

    def fwd(*a, **k):
        calls["fwd"] += 1
        return fwd0(*a, **k)

    def bwd(*a, **k):
        calls["bwd"] += 1
        return bwd0(*a, **k)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "ATTN_LONG", fused)
        mp.setattr(ops, "attention_fwd_dh", fwd)
        mp.setattr(ops, "attention_bwd_dh", bwd)
        vit = ViT(patch_size=16, q_format="FP32", precision="bf16", **kw)
        vit.load_state_dict(params)
        vit = vit.cuda()
        logits = vit(img.cuda())
        cross_entropy(logits, labels.cuda()).backward()
        torch.cuda.synchronize()
    grads = {k: p.grad.float().cpu() for k, p in vit.named_parameters() if p.grad is not None}
    return logits.float().cpu(), grads, calls


@pytest.mark.parametrize("dh", WIDTHS)
@pytest.mark.parametrize("decoder,image_size,num_classes", [("classification", 224, 45), ("segmentation", 384, 17)])
def test_bf16_model_matches_oracle_and_materialised_path(ops, monkeypatch, decoder, image_size, num_classes, dh):
    batch, name = 2, f"dh{dh}_{decoder}_{image_size}"
    kw = dict(decoder=decoder, image_size=image_size, num_classes=num_classes, **MODELS[dh])
    cfg = ViTConfig(patch_size=16, **kw)
    params = {k: det_param(k, s) for k, s in cfg.param_shapes().items()}
    img = det_images(name, batch, image_size)
    shape = (batch,) if decoder == "classification" else (batch, image_size, image_size)
    labels = det_labels(name, shape, num_classes)
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, img, labels, cfg)
    logits, grads, calls = _run_model(ops, kw, params, img, labels, monkeypatch, fused=True)
    assert calls == {"fwd": 2, "bwd": 2}                     # both layers ran the new kernels, forward and backward
    err = float((logits - ref_logits).abs().max() / ref_logits.abs().max())
    print(f"{name}: logits vs oracle {err:.3e}")
    assert err < 1.5e-2, err
    n, worst = 0, 0.0
    for k, gr in grads.items():
        if ref_grads.get(k) is None:
            continue
        e = relerr(gr, ref_grads[k])
        worst = max(worst, e)
        assert e < 2e-2, (k, e)
        n += 1
    print(f"{name}: worst gradient vs oracle {worst:.3e} over {n} tensors")
    assert n > 20
    # the same model on the materialised fp32 path: what these widths took before
    logits_m, grads_m, calls_m = _run_model(ops, kw, params, img, labels, monkeypatch, fused=False)
    assert calls_m == {"fwd": 0, "bwd": 0}
    err_m = float((logits - logits_m).abs().max() / logits_m.abs().max())
    worst_m = max(relerr(grads[k], grads_m[k]) for k in grads_m)
    print(f"{name}: vs materialised path: logits {err_m:.3e}, worst gradient {worst_m:.3e}")
    assert set(grads) == set(grads_m)
    assert err_m < 6e-3, err_m
    assert worst_m < 2e-2, worst_m
