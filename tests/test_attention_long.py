"""GPU: the key-tiled bf16 attention core for sequences longer than 320 tokens (mv_attention_fwd_long / _bwd_long).

ViT-B/16 at 384^2 has 577 tokens, patch 8 at 224^2 785, segmentation at 512^2 1 025: the whole-head kernels stop at 320.  The
kernels against fp64 (the bars of test_hip_ops.py::test_attention_fused_fwd_bwd), the long kernels at short lengths, determinism,
key-permutation invariance, the absence of any [B, H, N, N] tensor, whole models against the CPU oracle at the bf16 envelope,
graph capture, and the batch-decomposition properties of ViT-B/16 at 384^2."""
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


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def bf(x):
    return x.to(torch.bfloat16)


def attn_ref(qkv, H):
    B, N, _ = qkv.shape
    q, k, v = qkv.double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * SCALE
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * 64), torch.logsumexp(s, dim=-1)


def make(B, N, H, qk_mult=1.0, seed=1):
    qkv = torch.randn(B, N, 3, H, 64, generator=g(seed)) * 1.5
    qkv[:, :, :2] *= qk_mult
    return bf(qkv.view(B, N, 3 * H * 64)), bf(torch.randn(B, N, H * 64, generator=g(seed + 1)))


def check_against_fp64(ops, qkv, dout, B, N, H, fwd, bwd):
    ref_in = qkv.double().requires_grad_(True)
    want, lse_ref = attn_ref(ref_in, H)
    want.backward(dout.double())
    out, lse = fwd(qkv.cuda(), B, N, H, SCALE)
    # P is rounded to bf16 before P.V (2^-9 per element, averaged over keys) and the output once more
    assert relerr(out.float(), want) < 1.5e-2
    assert float((lse.cpu().double() - lse_ref.detach()).abs().max()) < 1e-4
    part = torch.full((B, 3 * H * 64), float("nan"), device="cuda")
    dqkv = bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, SCALE, colsum=part)
    got, ref = dqkv.float().cpu().view(B, N, 3, H, 64), ref_in.grad.view(B, N, 3, H, 64)
    for i, name in enumerate("qkv"):
        assert relerr(got[:, :, i], ref[:, :, i]) < 3e-2, name
    assert relerr(part.cpu(), dqkv.float().sum(1).cpu()) < 5e-3
    assert relerr(part.cpu().double(), ref_in.grad.sum(1)) < 3e-2
    dq2 = bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, SCALE)          # colsum is optional
    assert torch.equal(dq2, dqkv)
    return out, lse, dqkv, part


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 321, 2, 1.0), (1, 385, 3, 1.0), (2, 577, 2, 1.0), (1, 577, 2, 4.0),
                                           (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
def test_long_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult):
    """ops.attention_fwd / _bwd route N > 320 to the key-tiled kernels.  qk_mult = 4: scores 16x larger, so the running maximum
    of a query row really moves between key blocks and the accumulators are rescaled."""
    qkv, dout = make(B, N, H, qk_mult)
    check_against_fp64(ops, qkv, dout, B, N, H, ops.attention_fwd, ops.attention_bwd)


@pytest.mark.parametrize("B,N,H", [(3, 17, 2), (2, 197, 3), (1, 257, 2), (2, 320, 1)])
def test_long_kernels_at_short_lengths_vs_fp64(ops, B, N, H):
    qkv, dout = make(B, N, H, seed=5)
    check_against_fp64(ops, qkv, dout, B, N, H, ops.attention_fwd_long, ops.attention_bwd_long)


def test_short_lengths_keep_the_whole_head_kernels(ops):
    """N <= 320 still takes mv_attention_fwd / _bwd: ops.attention_fwd gives exactly their bits."""
    from myrtle_vision.hip.lib import lib
    B, N, H = 2, 197, 3
    qkv, dout = make(B, N, H, seed=7)
    qkv = qkv.cuda()
    out = torch.empty(B, N, H * 64, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    assert lib().mv_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, SCALE,
                                  torch.cuda.current_stream().cuda_stream) == 0
    out_d, lse_d = ops.attention_fwd(qkv, B, N, H, SCALE)
    assert torch.equal(out_d, out) and torch.equal(lse_d, lse)
    # the whole-head entry points keep their cap
    assert lib().mv_attention_fwd(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, 321, 1, SCALE,
                                  torch.cuda.current_stream().cuda_stream) != 0
    torch.cuda.synchronize()


def test_long_attention_is_deterministic(ops):
    B, N, H = 2, 1025, 3
    qkv, dout = make(B, N, H, seed=11)
    qkv, dout = qkv.cuda(), dout.cuda()
    runs = []
    for _ in range(2):
        out, lse = ops.attention_fwd(qkv, B, N, H, SCALE)
        part = torch.empty(B, 3 * H * 64, device="cuda")
        dqkv = ops.attention_bwd(qkv, out, dout, lse, B, N, H, SCALE, colsum=part)
        runs.append((out, lse, dqkv, part))
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def test_long_attention_key_permutation(ops):
    """Permuting keys and values together leaves softmax(QK^T)V unchanged up to the order of the fp32 sums and the bf16 rounding
    of P (which sees other running maxima); dK and dV permute with them, dQ stays."""
    B, N, H = 2, 577, 2
    qkv, dout = make(B, N, H, seed=13)
    qkv, dout = qkv.cuda(), dout.cuda()
    perm = torch.randperm(N, generator=g(14)).cuda()
    q5 = qkv.view(B, N, 3, H, 64)
    q5p = q5.clone()
    q5p[:, :, 1] = q5[:, perm, 1]
    q5p[:, :, 2] = q5[:, perm, 2]
    qkvp = q5p.view(B, N, 3 * H * 64).contiguous()
    out, lse = ops.attention_fwd(qkv, B, N, H, SCALE)
    out_p, lse_p = ops.attention_fwd(qkvp, B, N, H, SCALE)
    assert rel_l2(out_p.float(), out.float()) < 6e-3
    assert float((lse_p - lse).abs().max()) < 1e-4
    d = ops.attention_bwd(qkv, out, dout, lse, B, N, H, SCALE).float().view(B, N, 3, H, 64)
    dp = ops.attention_bwd(qkvp, out_p, dout, lse_p, B, N, H, SCALE).float().view(B, N, 3, H, 64)
    assert rel_l2(dp[:, :, 0], d[:, :, 0]) < 2e-2
    for i in (1, 2):
        assert rel_l2(dp[:, :, i], d[:, perm, i]) < 2e-2, "kv"[i - 1]


def test_attention_core_keeps_no_n_squared_tensor(ops):
    from myrtle_vision.hip import functional as F
    B, H, N = 8, 12, 1025
    qkv, dout = make(B, N, H, seed=17)
    qkv = qkv.cuda().requires_grad_(True)
    dout = dout.cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = F.attention_core(qkv, H, SCALE)
    out.backward(dout)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert qkv.grad is not None and bool(torch.isfinite(qkv.grad.float()).all())
    assert grew < B * H * N * N * 4 / 4, grew


# ---------------------------------------------------------------- models
def _model_vs_oracle(decoder, image_size, num_classes, batch, name):
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    kw = dict(decoder=decoder, image_size=image_size, num_classes=num_classes, dim=192, depth=2, heads=3, mlp_dim=768)
    cfg = ViTConfig(patch_size=16, **kw)
    params = {k: det_param(k, s) for k, s in cfg.param_shapes().items()}
    img = det_images(name, batch, image_size)
    shape = (batch,) if decoder == "classification" else (batch, image_size, image_size)
    labels = det_labels(name, shape, num_classes)
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, img, labels, cfg)
    vit = ViT(patch_size=16, q_format="FP32", precision="bf16", **kw)
    vit.load_state_dict(params)
    vit = vit.cuda()
    logits = vit(img.cuda())
    cross_entropy(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    err = float((logits.float().cpu() - ref_logits).abs().max() / ref_logits.abs().max())
    assert err < 1.5e-2, err
    n = 0
    for k, p in vit.named_parameters():
        if ref_grads[k] is None:
            continue
        e = rel_l2(p.grad.float().cpu(), ref_grads[k])
        assert e < 2e-2, (k, e)
        n += 1
    assert n > 20


def test_bf16_classification_384_matches_oracle(ops):
    _model_vs_oracle("classification", 384, 45, 2, "long_cls_384")


def test_bf16_segmentation_512_matches_oracle(ops):
    _model_vs_oracle("segmentation", 512, 17, 2, "long_seg_512")


def test_graphed_step_equals_eager_step_at_384(ops):
    """GraphedTrainStep at 577 tokens (the key-tiled kernels, their torch-allocated delta workspace inside the capture): the
    replays give the eager steps' losses and parameters bit for bit, as tests/test_train_gpu.py checks at 224^2."""
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
        vit = ViT(precision="bf16", q_format="FP32", **kw).cuda().train()
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


# ---------------------------------------------------------------- ViT-B/16 at 384^2, batch 64
@pytest.fixture(scope="module")
def vit_b384():
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(7)
    vit = ViT(precision="bf16", q_format="FP32", decoder="classification", image_size=384, patch_size=16, num_classes=1000,
              dim=768, depth=12, heads=12, mlp_dim=3072, dropout=0.0, emb_dropout=0.0).cuda()
    vit.train()
    return vit


def _grads(vit, img, labels):
    from myrtle_vision.hip.functional import cross_entropy
    for p in vit.parameters():
        p.grad = None
    loss = cross_entropy(vit(img), labels)
    loss.backward()
    skip = set(vit.unused_parameter_names())
    return float(loss.detach()), {n: p.grad.detach().clone() for n, p in vit.named_parameters() if n not in skip and p.grad is not None}


def test_vit_b_384_logits_are_per_sample_independent(vit_b384):
    img = torch.randn(64, 3, 384, 384, generator=g(11)).cuda()
    with torch.no_grad():
        full = vit_b384(img).float()
        part = vit_b384(img[40:48].contiguous()).float()
    assert rel_l2(full[40:48], part) < 1e-5
    assert torch.equal(full[40:48].argmax(1), part.argmax(1))


def test_vit_b_384_gradient_is_the_mean_of_its_halves(vit_b384):
    img = torch.randn(64, 3, 384, 384, generator=g(12)).cuda()
    labels = torch.randint(0, 1000, (64,), generator=g(13)).cuda()
    loss, full = _grads(vit_b384, img, labels)
    l0, h0 = _grads(vit_b384, img[:32].contiguous(), labels[:32].contiguous())
    l1, h1 = _grads(vit_b384, img[32:].contiguous(), labels[32:].contiguous())
    assert abs(loss - 0.5 * (l0 + l1)) < 1e-5 * abs(loss)
    assert set(full) == set(h0) == set(h1) and len(full) > 140
    worst = max(rel_l2(0.5 * (h0[n] + h1[n]), full[n]) for n in full)
    assert worst < 2e-4, worst
