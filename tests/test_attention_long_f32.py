"""GPU: the key-tiled exact-fp32 attention core past 272 tokens (mv_attention_fwd_long_f32 / _f32_q8 / mv_attention_bwd_long_f32),
the core of precisions "fp32" and "bf16x3" and of the converted int8 model.

The kernels against fp64 at the bars of test_hip_ops.py::test_attention_fused_fp32_forward / _backward, through the dispatch and
called directly at short lengths; agreement with the materialised fp32 path; determinism; key-permutation invariance; the int8
codes of the quantiser-fused form; the absence of any [B, H, N, N] tensor; fp32 and bf16x3 models at 384^2 and 512^2 against the
CPU oracle and against the materialised path; the converted int8 model at 384^2; graph capture."""
import numpy as np
import pytest
import torch

from oracle import int8_oracle
from oracle.detinit import det_images, det_labels, det_param, det_state_dict
from oracle.vit_oracle import ViTConfig, loss_and_grads
from test_vit_parity import report

pytestmark = pytest.mark.gpu

SCALE = 64 ** -0.5
OUT_BAR, LSE_BAR, GRAD_BAR, SPIKE_BAR = 2e-6, 2e-5, 5e-6, 5e-5      # test_hip_ops.py's fp32 attention bars


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


def make(B, N, H, qk_mult=1.0, seed=1):
    """-> (fp32 qkv [B, N, 3*H*64], fp32 dout [B, N, H*64]) on the host; qk_mult scales q and k (scores by qk_mult^2)"""
    qkv = torch.randn(B, N, 3, H, 64, generator=g(seed)) * 1.5
    qkv[:, :, :2] *= qk_mult
    return qkv.view(B, N, 3 * H * 64), torch.randn(B, N, H * 64, generator=g(seed + 1))


def grad_errs(got, ref, B, N, H):
    """Per-part (q, k, v) relative L2 errors.  A part that is exactly zero in exact arithmetic (dq, dk at N = 1, where softmax is
    exactly 1) is held against the size of the whole gradient instead of its own."""
    got, ref = got.detach().double().cpu().view(B, N, 3, H, 64), ref.detach().double().cpu().view(B, N, 3, H, 64)
    errs = []
    for i in range(3):
        den = float(ref[:, :, i].norm())
        if den <= 1e-3 * float(ref.norm()):
            den = float(ref.norm())
        errs.append(float((got[:, :, i] - ref[:, :, i]).norm()) / den)
    return errs


def materialised(ops, qkv_d, dout_d, B, N, H):
    probs = ops.attention_probs_fp32(qkv_d, B, N, H, 64, SCALE)
    out = ops.attention_pv_fp32(probs, qkv_d, B, N, H, 64)
    dqkv = ops.attention_bwd_fp32(probs, qkv_d, dout_d, B, N, H, 64, SCALE)
    return out, dqkv


def check_against_fp64(ops, qkv, dout, B, N, H, fwd_lse, fwd_plain, bwd, vs_materialised):
    ref_in = qkv.double().requires_grad_(True)
    want, lse_ref = attn_ref(ref_in, H)
    want.backward(dout.double())
    qkv_d, dout_d = qkv.cuda(), dout.cuda()
    bars = dict(out=OUT_BAR, lse=LSE_BAR, grad=GRAD_BAR)
    mat = materialised(ops, qkv_d, dout_d, B, N, H) if vs_materialised else None
    if N == 4097:
        # at this length only: the larger of the bar and twice the materialised fp32 path's own error against fp64 (same input);
        # the lse bar stays (the materialised path has no lse)
        bars["out"] = max(OUT_BAR, 2 * relerr(mat[0], want))
        bars["grad"] = max(GRAD_BAR, 2 * max(grad_errs(mat[1], ref_in.grad, B, N, H)))
    out, lse = fwd_lse(qkv_d, B, N, H, SCALE)
    assert out.dtype == torch.float32 and out.shape == (B, N, H * 64) and lse.shape == (B, H, N)
    e_out = relerr(out, want)
    e_lse = float((lse.cpu().double() - lse_ref.detach()).abs().max())
    assert e_out < bars["out"], (e_out, bars)
    assert e_lse < bars["lse"], e_lse
    plain = fwd_plain(qkv_d, B, N, H, SCALE)
    assert torch.equal(plain, out)                                    # the evaluation form: the same bits without the lse
    assert torch.equal(fwd_lse(qkv_d, B, N, H, SCALE)[0], out)        # deterministic
    dqkv = bwd(qkv_d, out, dout_d, lse, B, N, H, SCALE)
    assert dqkv.dtype == torch.float32 and dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv).all())
    errs = grad_errs(dqkv, ref_in.grad, B, N, H)
    assert max(errs) < bars["grad"], (errs, bars)
    assert torch.equal(bwd(qkv_d, out, dout_d, lse, B, N, H, SCALE), dqkv)     # deterministic
    if mat is not None:                                               # the materialised fp32 path at the same bars
        assert relerr(out, mat[0]) < bars["out"]
        assert max(grad_errs(dqkv, mat[1], B, N, H)) < bars["grad"]
    report(f"attn_long_f32 N={N} out / lse / dq dk dv vs fp64", max([e_out] + errs))
    return out, lse, dqkv


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 273, 2, 1.0), (2, 289, 2, 1.0), (1, 321, 3, 1.0), (2, 577, 2, 1.0), (1, 577, 2, 2.0),
                                           (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
def test_long_fp32_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult):
    """ops.attention_fwd_f32_lse / attention_fwd_f32 / attention_bwd_f32_fused route N > 272 to the key-tiled kernels.  qk_mult = 2:
    scores 4x larger, so the running maximum of a query row moves between key blocks and the accumulators are rescaled."""
    qkv, dout = make(B, N, H, qk_mult)
    check_against_fp64(ops, qkv, dout, B, N, H, ops.attention_fwd_f32_lse, ops.attention_fwd_f32, ops.attention_bwd_f32_fused,
                       vs_materialised=True)


@pytest.mark.parametrize("B,N,H", [(3, 1, 2), (3, 17, 2), (2, 197, 3), (1, 272, 2)])
def test_long_fp32_kernels_at_short_lengths_vs_fp64(ops, B, N, H):
    """The long kernels called directly where the whole-head kernels run: one row, a ragged single block, 197 and 272 tokens."""
    qkv, dout = make(B, N, H, seed=5)
    check_against_fp64(ops, qkv, dout, B, N, H, ops.attention_fwd_long_f32,
                       lambda *a: ops.attention_fwd_long_f32(*a, lse=False), ops.attention_bwd_long_f32, vs_materialised=False)


def test_long_fp32_attention_spiked_score(ops):
    """One query whose scores are ~30x the rest (scores of ~ +-300: one fp32 ulp of the score is 3e-5 in the exponent)."""
    B, N, H = 2, 577, 2
    qkv, dout = make(B, N, H, seed=9)
    qkv = qkv.clone()
    qkv[0, 3, :64] *= 30.0
    ref_in = qkv.double().requires_grad_(True)
    want, _ = attn_ref(ref_in, H)
    want.backward(dout.double())
    out, lse = ops.attention_fwd_f32_lse(qkv.cuda(), B, N, H, SCALE)
    assert relerr(out, want) < SPIKE_BAR
    dqkv = ops.attention_bwd_f32_fused(qkv.cuda(), out, dout.cuda(), lse, B, N, H, SCALE)
    assert max(grad_errs(dqkv, ref_in.grad, B, N, H)) < SPIKE_BAR


def test_short_lengths_keep_the_whole_head_fp32_kernels(ops):
    """At N <= 272 the wrappers call exactly what they called before: the whole-head kernels' bits."""
    from myrtle_vision.hip.lib import lib
    B, N, H = 2, 257, 2
    qkv, dout = make(B, N, H, seed=3)
    qkv_d, dout_d = qkv.cuda(), dout.cuda()
    out, lse = ops.attention_fwd_f32_lse(qkv_d, B, N, H, SCALE)
    out2, lse2 = torch.empty_like(out), torch.empty_like(lse)
    assert lib().mv_attention_fwd_f32_lse(qkv_d.data_ptr(), out2.data_ptr(), lse2.data_ptr(), B, N, H, SCALE, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    dqkv = ops.attention_bwd_f32_fused(qkv_d, out, dout_d, lse, B, N, H, SCALE)
    d2 = torch.empty_like(qkv_d)
    assert lib().mv_attention_bwd_f32(qkv_d.data_ptr(), out.data_ptr(), dout_d.data_ptr(), lse.data_ptr(), d2.data_ptr(), B, N, H,
                                      SCALE, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(dqkv, d2)


def test_long_fp32_attention_key_permutation(ops):
    """Permuting keys and values together leaves out, lse and dq unchanged up to the order of the fp32 sums, and permutes dk / dv."""
    B, N, H = 2, 577, 2
    qkv, dout = make(B, N, H, seed=13)
    perm = torch.randperm(N, generator=g(14))
    qkvp = qkv.view(B, N, 3, H * 64).clone()
    qkvp[:, :, 1:] = qkvp[:, perm, 1:]
    qkvp = qkvp.view(B, N, 3 * H * 64)
    outs = []
    for x in (qkv, qkvp):
        xd = x.cuda()
        out, lse = ops.attention_fwd_f32_lse(xd, B, N, H, SCALE)
        outs.append((out, lse, ops.attention_bwd_f32_fused(xd, out, dout.cuda(), lse, B, N, H, SCALE)))
    (o, l, d), (op, lp, dp) = outs
    assert relerr(op, o) < OUT_BAR
    assert float((lp - l).abs().max()) < LSE_BAR
    d, dp = d.view(B, N, 3, H * 64), dp.view(B, N, 3, H * 64)
    assert relerr(dp[:, :, 0], d[:, :, 0]) < GRAD_BAR
    for i in (1, 2):
        assert relerr(dp[:, :, i], d[:, perm, i]) < GRAD_BAR, "kv"[i - 1]


@pytest.mark.parametrize("N", [577, 1025])
def test_long_fp32_q8_codes_equal_quantised_output(ops, N):
    """The quantiser-fused forward of the converted int8 model: its codes are quant_affine_i8 of the plain output, bit for bit."""
    B, H = 2, 3
    qkv, _ = make(B, N, H, seed=21)
    qkv_d = qkv.cuda()
    o = ops.attention_fwd_f32(qkv_d, B, N, H, SCALE)
    for s2, z2 in ((0.004, 131), (0.0125, 0), (0.002, 255)):
        codes = ops.attention_fwd_f32_q8(qkv_d, B, N, H, SCALE, s2, z2)
        assert torch.equal(codes.view(B * N, H * 64), ops.quant_affine_i8(o.view(B * N, H * 64), B * N, H * 64, s2, z2))


def test_long_fp32_attention_keeps_no_n_squared_tensor(ops):
    """ViT-B heads at 1 025 tokens (512^2 segmentation), batch 8: attention_core forward + backward on fp32 q/k/v allocates less
    than half of one [B, H, N, N] fp32 tensor (403 MB); the materialised path holds the probabilities and a dP of that size."""
    from myrtle_vision.hip import functional as F
    B, H, N = 8, 12, 1025
    qkv, dout = make(B, N, H, seed=17)
    qkv = qkv.cuda().requires_grad_(True)
    dout = dout.cuda()
    half = B * H * N * N * 4 / 2
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = F.attention_core(qkv, H, SCALE, None)
    out.backward(dout)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert bool(torch.isfinite(qkv.grad).all())
    assert grew < half, (grew, half)


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


def _run_fused_only(ops, vit, img, labels):
    """One training step in which the materialised attention must not run (ops.attention_probs_fp32 raises)."""
    def no_probs(*a, **k):
        raise AssertionError("materialised attention ran")

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ops, "ATTN_LONG", True)
        mp.setattr(ops, "attention_probs_fp32", no_probs)
        return _run(vit, img, labels)
    finally:
        mp.undo()


def test_fp32_model_at_384_never_materialises(ops):
    _, params, img, labels = _case("classification", 384, 45, 2, "long_cls_384")
    logits, grads = _run_fused_only(ops, _model("classification", 384, 45, "fp32", params), img, labels)
    assert bool(torch.isfinite(logits).all()) and len(grads) > 20


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("decoder,image_size,num_classes,name", [("classification", 384, 45, "long_cls_384"),
                                                                  ("segmentation", 512, 17, "long_seg_512")])
def test_exact_modes_with_long_fp32_attention_match_oracle(ops, precision, decoder, image_size, num_classes, name):
    """fp32 and bf16x3 at the north-star contract (1e-3 on the logits, 1e-3 relative L2 on every gradient tensor), every block's
    attention on the key-tiled fp32 kernels (no fall-back)."""
    cfg, params, img, labels = _case(decoder, image_size, num_classes, 2, name)
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, img, labels, cfg)
    logits, grads = _run_fused_only(ops, _model(decoder, image_size, num_classes, precision, params), img, labels)
    err = float((logits - ref_logits).abs().max() / ref_logits.abs().max())
    report(f"attn_long_f32 {precision} {decoder} {image_size} logits vs oracle", err)
    assert err < 1e-3, err
    worst, n = 0.0, 0
    for k, gr in grads.items():
        if ref_grads[k] is None:
            continue
        e = relerr(gr, ref_grads[k])
        assert e < 1e-3, (k, e)
        worst, n = max(worst, e), n + 1
    report(f"attn_long_f32 {precision} {decoder} {image_size} worst gradient vs oracle", worst)
    assert n > 20


@pytest.mark.parametrize("decoder,image_size,num_classes,name", [("classification", 384, 45, "long_cls_384"),
                                                                  ("segmentation", 512, 17, "long_seg_512")])
def test_fp32_model_long_attention_vs_materialised(ops, decoder, image_size, num_classes, name):
    """The fp32 mode with ATTN_LONG off (materialised attention) and on (key-tiled) in one process: logits within 1e-5 of
    max |logit|, every gradient tensor within 1e-4 relative L2."""
    _, params, img, labels = _case(decoder, image_size, num_classes, 2, name)
    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(ops, "ATTN_LONG", False)
        l_mat, g_mat = _run(_model(decoder, image_size, num_classes, "fp32", params), img, labels)
    finally:
        mp.undo()
    l_long, g_long = _run_fused_only(ops, _model(decoder, image_size, num_classes, "fp32", params), img, labels)
    err = float((l_long - l_mat).abs().max() / l_mat.abs().max())
    report(f"attn_long_f32 fp32 {decoder} {image_size} logits long vs materialised", err)
    assert err < 1e-5, err
    assert set(g_long) == set(g_mat) and len(g_mat) > 20
    worst = max(relerr(g_long[k], g_mat[k]) for k in g_mat)
    report(f"attn_long_f32 fp32 {decoder} {image_size} worst gradient long vs materialised", worst)
    assert worst < 1e-4, worst


def test_converted_int8_model_at_384_uses_the_fused_core(ops):
    """A converted PyTorchINT8 small model at 384^2 (577 tokens): every attention block takes int8_fused_forward (the fused
    exact-fp32 core with to_out's quantiser folded in), and the logits match the int8 oracle at test_int8_model.py's micro bar.
    Width 256 / 4 heads rather than the micro model's 192 / 3: the int8 matrix-core GEMM that the fused block feeds takes K in
    multiples of 256 (ops.linear_i8_supported), so at width 192 no block is fusable at any length."""
    from myrtle_vision.models import vit as vit_mod
    from myrtle_vision.models.vit import ViT
    kw = dict(decoder="classification", image_size=384, patch_size=16, num_classes=45, dim=256, depth=2, heads=4, mlp_dim=1024)
    calib = [det_images(f"int8-calib384-{i}", 4, 384) for i in range(3)]
    img = det_images("int8-eval384", 4, 384)
    cfg = ViTConfig(**kw)
    params = det_state_dict(cfg.param_shapes())
    vit = ViT(q_format="FP32", precision="bf16", **kw)
    vit.load_state_dict(params)
    vit = vit.cuda()
    vit.quantizer.prepare_qat("PyTorchINT8")
    with torch.no_grad():
        for b in calib:
            vit(b.cuda())
    vit.convert()
    vit.eval()
    calls = {"fused": 0, "none": 0}
    real = vit_mod.Attention.int8_fused_forward

    def counting(self, x, norm):
        r = real(self, x, norm)
        calls["fused" if r is not None else "none"] += 1
        return r

    mp = pytest.MonkeyPatch()
    try:
        mp.setattr(vit_mod.Attention, "int8_fused_forward", counting)
        with torch.no_grad():
            got = vit(img.cuda()).float().cpu().numpy()
    finally:
        mp.undo()
    assert calls == {"fused": cfg.depth, "none": 0}, calls
    torch.set_num_threads(8)
    ranges = int8_oracle.calibrate(params, calib, cfg)
    want = int8_oracle.int8_forward(params, img, cfg, int8_oracle.qparams(ranges)).numpy()
    scale = np.abs(want).max()
    err = float(np.abs(got - want).max() / scale)
    report("attn_long_f32 int8/micro 384 converted logits vs oracle", err)
    assert np.isfinite(got).all() and err < 1.5e-2, err
    top2 = np.sort(want, axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) / scale > 2 * err
    assert (got.argmax(1) == want.argmax(1))[safe].all()


def test_graphed_fp32_step_equals_eager_step_at_384(ops):
    """GraphedTrainStep at 577 tokens in fp32 (the key-tiled fp32 kernels and their torch-allocated delta workspace inside the
    capture): the replays give the eager steps' losses and parameters bit for bit."""
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
        vit = ViT(precision="fp32", q_format="FP32", **kw).cuda().train()
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
