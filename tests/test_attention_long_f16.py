"""GPU: the key-tiled half-operand attention core of precision "bf16x3h" past 288 tokens (mv_attention_fwd_long_f16 / _bwd_long_f16).

The kernels against fp64 on the SAME half-rounded q/k/v (the bars of test_hip_ops.py::test_attention_f16_fwd_bwd) through the
dispatch and called directly at short lengths, at three gradient magnitudes; the split-operand outputs and column sums; determinism;
exact zeros; key-permutation invariance; the absence of any [B, H, N, N] tensor; bf16x3h models at 384^2 and 512^2 against the CPU
oracle at the precision's own 1e-3 bar and against the fp32 mode; batch independence of ViT-B/16 at 384^2; graph capture."""
import pytest
import torch

from oracle.detinit import det_images, det_labels, det_param
from oracle.vit_oracle import ViTConfig, loss_and_grads

pytestmark = pytest.mark.gpu

SCALE = 64 ** -0.5


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


def attn_ref(qkv, H):
    B, N, _ = qkv.shape
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * 64), torch.logsumexp(s, dim=-1)


def make(ops, B, N, H, gscale=1.0, qk_mult=1.0, seed=1):
    """-> (half q/k/v on the device, fp32 dout on the host)"""
    qkv = torch.randn(B, N, 3, H, 64, generator=g(seed)) * 1.2
    qkv[:, :, :2] *= qk_mult
    q16 = ops.cast_f16(qkv.view(B, N, 3 * H * 64).cuda())
    return q16, torch.randn(B, N, H * 64, generator=g(seed + 1)) * gscale


def check_against_fp64(ops, q16, dout, B, N, H, fwd, bwd):
    ref_in = q16.cpu().double().requires_grad_(True)
    want, lse_ref = attn_ref(ref_in, H)
    want.backward(dout.double())
    out, lse = fwd(q16, B, N, H, SCALE)
    assert out.dtype == torch.float32 and relerr(out, want) < 6e-4, relerr(out, want)
    assert float((lse.cpu().double() - lse_ref.detach()).abs().max()) < 2e-5
    dqkv = bwd(q16, out, dout.cuda(), lse, B, N, H, SCALE)
    assert dqkv.dtype == torch.float32 and bool(torch.isfinite(dqkv).all())
    got, ref = dqkv.cpu().double().view(B, N, 3, H, 64), ref_in.grad.view(B, N, 3, H, 64)
    for i, name in enumerate("qkv"):
        # (N = 1: softmax is exactly 1, so dq = dk = 0 exactly; the kernels leave rounding residue of P - 1 and dP - delta, held
        # here against the size of the whole gradient)
        e = float((got[:, :, i] - ref[:, :, i]).norm() / max(float(ref[:, :, i].norm()), 1e-3 * float(ref.norm())))
        assert e < 2e-3, (name, e)
    # the split-output form (what the bf16x3h block runs): the bf16 pieces of exactly those fp32 values, and per-image column sums
    for nseg in (3, 6):
        with ops.segments(nseg):
            part = torch.full((B, 3 * H * 64), float("nan"), device="cuda")
            pieces = bwd(q16, out, dout.cuda(), lse, B, N, H, SCALE, split=True, colsum=part)
            assert torch.equal(pieces, ops.split_ex(dqkv.view(B * N, 3 * H * 64), B * N, 3 * H * 64))
        assert relerr(part, dqkv.double().sum(1)) < 1e-5
    part = torch.full((B, 3 * H * 64), float("nan"), device="cuda")
    assert torch.equal(bwd(q16, out, dout.cuda(), lse, B, N, H, SCALE, colsum=part), dqkv)   # colsum is optional; deterministic
    assert relerr(part, dqkv.double().sum(1)) < 1e-5
    # an all-zero gradient gives exact zeros (scale 1, no 0 * inf)
    assert not bwd(q16, out, torch.zeros_like(dout).cuda(), lse, B, N, H, SCALE).any()
    return out, lse, dqkv


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 289, 2, 1.0), (1, 300, 3, 1.0), (2, 321, 1, 1.0), (2, 577, 2, 1.0), (1, 577, 2, 3.0),
                                           (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
@pytest.mark.parametrize("gscale", [1.0, 3.0e-7, 4.0e4])
def test_long_half_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult, gscale):
    """ops.attention_fwd_f16 / _bwd_f16 route N > 288 to the key-tiled half kernels.  qk_mult = 3: scores 9x larger, so the running
    maximum of a query row moves between key blocks and the accumulators are rescaled.  The gradient magnitudes: O(1), far below
    half's normal range and above half's largest value divided by the key count -- the same relative error at each."""
    q16, dout = make(ops, B, N, H, gscale, qk_mult)
    check_against_fp64(ops, q16, dout, B, N, H, ops.attention_fwd_f16, ops.attention_bwd_f16)


@pytest.mark.parametrize("B,N,H", [(3, 1, 2), (3, 17, 2), (2, 64, 1), (2, 197, 3), (1, 257, 2)])
@pytest.mark.parametrize("gscale", [1.0, 3.0e-7, 4.0e4])
def test_long_half_kernels_at_short_lengths_vs_fp64(ops, B, N, H, gscale):
    """The long half kernels called directly where the whole-head kernels would run: one row, ragged blocks, exactly one block."""
    q16, dout = make(ops, B, N, H, gscale, seed=5)
    check_against_fp64(ops, q16, dout, B, N, H, ops.attention_fwd_long_f16, ops.attention_bwd_long_f16)


def test_short_lengths_keep_the_whole_head_half_kernels(ops):
    """N <= 288 still takes mv_attention_fwd_f16 / _bwd_f16: the dispatch gives exactly their bits, and they keep their cap."""
    from myrtle_vision.hip.lib import lib
    B, N, H = 2, 257, 3
    q16, dout = make(ops, B, N, H, seed=7)
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, N, H * 64, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    assert lib().mv_attention_fwd_f16(q16.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, SCALE, st) == 0
    out_d, lse_d = ops.attention_fwd_f16(q16, B, N, H, SCALE)
    assert torch.equal(out_d, out) and torch.equal(lse_d, lse)
    assert lib().mv_attention_fwd_f16(q16.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, 289, 1, SCALE, st) != 0
    torch.cuda.synchronize()


def test_long_half_attention_is_deterministic(ops):
    B, N, H = 2, 1025, 3
    q16, dout = make(ops, B, N, H, seed=11)
    dout = dout.cuda()
    runs = []
    for _ in range(2):
        out, lse = ops.attention_fwd_f16(q16, B, N, H, SCALE)
        part = torch.empty(B, 3 * H * 64, device="cuda")
        with ops.segments(3):
            pieces = ops.attention_bwd_f16(q16, out, dout, lse, B, N, H, SCALE, split=True, colsum=part)
        runs.append((out, lse, pieces.view(torch.int16), part))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_long_half_attention_key_permutation(ops):
    """Permuting keys and values together leaves softmax(QK^T)V unchanged up to the order of the fp32 sums and the half rounding of
    P (which sees other running maxima); dK and dV permute with them, dQ stays."""
    B, N, H = 2, 577, 2
    q16, dout = make(ops, B, N, H, seed=13)
    dout = dout.cuda()
    perm = torch.randperm(N, generator=g(14)).cuda()
    q5 = q16.view(B, N, 3, H, 64)
    q5p = q5.clone()
    q5p[:, :, 1] = q5[:, perm, 1]
    q5p[:, :, 2] = q5[:, perm, 2]
    qp = q5p.view(B, N, 3 * H * 64).contiguous()
    out, lse = ops.attention_fwd_f16(q16, B, N, H, SCALE)
    out_p, lse_p = ops.attention_fwd_f16(qp, B, N, H, SCALE)
    assert relerr(out_p, out) < 6e-4
    assert float((lse_p - lse).abs().max()) < 2e-5
    d = ops.attention_bwd_f16(q16, out, dout, lse, B, N, H, SCALE).view(B, N, 3, H, 64)
    dp = ops.attention_bwd_f16(qp, out_p, dout, lse_p, B, N, H, SCALE).view(B, N, 3, H, 64)
    assert relerr(dp[:, :, 0], d[:, :, 0]) < 3e-3
    for i in (1, 2):
        assert relerr(dp[:, :, i], d[:, perm, i]) < 3e-3, "kv"[i - 1]


def test_long_half_attention_keeps_no_n_squared_tensor(ops):
    """ViT-B heads at 1 025 tokens (512^2 segmentation), batch 8: neither the forward nor the backward (fp32 dqkv and its column
    sums) allocates anything near one [B, H, N, N] fp32 tensor (403 MB); the materialised path holds three."""
    B, H, N = 8, 12, 1025
    q16, dout = make(ops, B, N, H, seed=17)
    dout = dout.cuda()
    part = torch.empty(B, 3 * H * 64, device="cuda")
    quarter = B * H * N * N * 4 / 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, lse = ops.attention_fwd_f16(q16, B, N, H, SCALE)
    torch.cuda.synchronize()
    grew_fwd = torch.cuda.max_memory_allocated() - base
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    dqkv = ops.attention_bwd_f16(q16, out, dout, lse, B, N, H, SCALE, colsum=part)
    torch.cuda.synchronize()
    grew_bwd = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(part).all())
    assert grew_fwd < quarter and grew_bwd < quarter, (grew_fwd, grew_bwd, quarter)


# ---------------------------------------------------------------- models
def _model(decoder, image_size, num_classes, precision, params):
    from myrtle_vision.models.vit import ViT
    vit = ViT(patch_size=16, q_format="FP32", precision=precision, decoder=decoder, image_size=image_size, num_classes=num_classes,
              dim=192, depth=2, heads=3, mlp_dim=768)
    vit.load_state_dict(params)
    return vit.cuda()


def _run(vit, img, labels):
    from myrtle_vision.hip.functional import cross_entropy
    logits = vit(img.cuda())
    cross_entropy(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    return logits.detach().float().cpu(), {k: p.grad.float().cpu() for k, p in vit.named_parameters() if p.grad is not None}


def _case(decoder, image_size, num_classes, batch, name):
    kw = dict(decoder=decoder, image_size=image_size, num_classes=num_classes, dim=192, depth=2, heads=3, mlp_dim=768)
    cfg = ViTConfig(patch_size=16, **kw)
    params = {k: det_param(k, s) for k, s in cfg.param_shapes().items()}
    img = det_images(name, batch, image_size)
    shape = (batch,) if decoder == "classification" else (batch, image_size, image_size)
    labels = det_labels(name, shape, num_classes)
    return cfg, params, img, labels


def _half_model_vs_oracle(ops, decoder, image_size, num_classes, batch, name):
    """bf16x3h at its own contract (1e-3 on the logits, 1e-3 relative L2 on every gradient tensor); the attention of every block
    takes the long half kernels (no fall-back: attention_probs_fp32 must not run)."""
    cfg, params, img, labels = _case(decoder, image_size, num_classes, batch, name)
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, img, labels, cfg)
    vit = _model(decoder, image_size, num_classes, "bf16x3h", params)
    calls = {"long": 0}
    real_fwd, real_probs = ops.attention_fwd_long_f16, ops.attention_probs_fp32

    def counting_fwd(*a, **k):
        calls["long"] += 1
        return real_fwd(*a, **k)

    def no_probs(*a, **k):
        raise AssertionError("materialised attention ran")

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ops, "attention_fwd_long_f16", counting_fwd)
        mp.setattr(ops, "attention_probs_fp32", no_probs)
        logits, grads = _run(vit, img, labels)
    finally:
        mp.undo()
    assert calls["long"] == 2
    err = float((logits - ref_logits).abs().max() / ref_logits.abs().max())
    assert err < 1e-3, err
    n = 0
    for k, gr in grads.items():
        if ref_grads[k] is None:
            continue
        e = relerr(gr, ref_grads[k])
        assert e < 1e-3, (k, e)
        n += 1
    assert n > 20


def test_bf16x3h_classification_384_matches_oracle(ops):
    _half_model_vs_oracle(ops, "classification", 384, 45, 2, "long_cls_384")


def test_bf16x3h_segmentation_512_matches_oracle(ops):
    _half_model_vs_oracle(ops, "segmentation", 512, 17, 2, "long_seg_512")


def test_bf16x3h_vs_fp32_full_tensors_at_384(ops):
    """Every element of every gradient tensor of bf16x3h against the fp32 mode (which materialises at 577 tokens), 1e-3 relative
    L2 per tensor and 1e-3 on the logits: test_vit_parity.py's bf16x3h_vs_fp32_full_tensors at 384^2."""
    _, params, img, labels = _case("classification", 384, 45, 2, "long_cls_384")
    l32, g32 = _run(_model("classification", 384, 45, "fp32", params), img, labels)
    lh, gh = _run(_model("classification", 384, 45, "bf16x3h", params), img, labels)
    assert float((lh - l32).abs().max() / l32.abs().max()) < 1e-3
    assert set(gh) == set(g32) and len(g32) > 20
    for k, ref in g32.items():
        e = relerr(gh[k], ref)
        assert e < 1e-3, (k, e)


def test_vit_b_384_bf16x3h_logits_are_per_sample_independent(ops):
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(7)
    vit = ViT(precision="bf16x3h", q_format="FP32", decoder="classification", image_size=384, patch_size=16, num_classes=1000,
              dim=768, depth=12, heads=12, mlp_dim=3072, dropout=0.0, emb_dropout=0.0).cuda().train()
    img = torch.randn(64, 3, 384, 384, generator=g(11)).cuda()
    with torch.no_grad():
        full = vit(img).float()
        part = vit(img[40:48].contiguous()).float()
    assert relerr(full[40:48], part) < 2e-3
    assert float((full[40:48] - part).abs().max() / part.abs().max()) < 2e-3


def test_graphed_bf16x3h_step_equals_eager_step_at_384(ops):
    """GraphedTrainStep at 577 tokens in bf16x3h (the long half kernels, their torch-allocated prep outputs and column-sum
    workspace inside the capture): the replays give the eager steps' losses and parameters bit for bit."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import AdamW, ParamArena
    from myrtle_vision.utils.utils import seed_everything
    kw = dict(decoder="classification", num_classes=10, image_size=384, patch_size=16, dim=128, depth=2, heads=2, mlp_dim=256,
              dropout=0.0, emb_dropout=0.0)

    def loss_fn(m, x, y):
        return cross_entropy(m(x), y)

    gen = g(9)
    batches = [(torch.randn(4, 3, 384, 384, generator=gen).cuda(), torch.randint(0, 10, (4,), generator=gen).cuda())
               for _ in range(4)]
    lrs = [1e-3, 1e-3, 4e-4, 7e-4]

    def build():
        seed_everything(21)
        vit = ViT(precision="bf16x3h", q_format="FP32", **kw).cuda().train()
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05)
        opt.max_grad_norm = 1.0
        return vit, opt

    def set_lr(opt, lr):
        for grp in opt.param_groups:
            grp["lr"] = lr

    vit_e, opt_e = build()
    losses_e = []
    for i in [0, 0, 0, 1, 2, 3]:
        set_lr(opt_e, lrs[i])
        opt_e.zero_grad()
        loss = loss_fn(vit_e, *batches[i])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
    vit_g, opt_g = build()
    graphed = GraphedTrainStep(vit_g, opt_g, loss_fn, *batches[0], warmup=3)
    losses_g = []
    for i in (1, 2, 3):
        set_lr(opt_g, lrs[i])
        losses_g.append(float(graphed(*batches[i])))
    torch.cuda.synchronize()
    assert opt_g.step_count == opt_e.step_count == 6
    assert losses_g == losses_e[3:]
    assert torch.equal(opt_g.arena.flat_param, opt_e.arena.flat_param)
