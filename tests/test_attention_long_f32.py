"""GPU: the key-tiled exact-fp32 attention core past 272 tokens (mv_attention_fwd_long_f32 / _f32_q8 / mv_attention_bwd_long_f32),
the core of precisions "fp32" and "bf16x3" and of the converted int8 model.

The kernels against fp64 through the dispatch and called directly at short lengths; agreement with the materialised fp32 path;
determinism; key-permutation invariance; the int8 codes of the quantiser-fused form; the absence of any [B, H, N, N] tensor; fp32
and bf16x3 models at 384^2 and 512^2 against the CPU oracle and against the materialised path; the converted int8 model at 384^2;
graph capture.  Bars, builders and the bodies shared with the other families: tests/attention_families.py (family "fp32")."""
import numpy as np
import pytest
import torch

pytest.register_assert_rewrite("attention_families")   # its shared bodies assert: failures show the values
from attention_families import (CLS_384, FAMILIES, INT8_MICRO_BAR, SEG_512, WATCH, assert_long_vs_materialised, attn_ref, build_model,
                                check_against_fp64, check_key_permutation, check_model_matches_oracle, check_no_n_squared_tensor,
                                check_short_lengths_keep_the_whole_head_kernels, grad_errs, graphed_step_equals_eager, make, model_case,
                                ops, relerr, report, run_model, watching)  # noqa: F401
from oracle import int8_oracle
from oracle.detinit import det_images, det_state_dict
from oracle.vit_oracle import ViTConfig

pytestmark = pytest.mark.gpu

FAM = FAMILIES["fp32"]
MODEL_CASES = [CLS_384, SEG_512]


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 273, 2, 1.0), (2, 289, 2, 1.0), (1, 321, 3, 1.0), (2, 577, 2, 1.0),
                                           (1, 577, 2, FAM.qk_mult), (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
def test_long_fp32_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult):
    """ops.attention_fwd_f32_lse / attention_fwd_f32 / attention_bwd_f32_fused route N > 272 to the key-tiled kernels.  qk_mult = 2:
    scores 4x larger, so the running maximum of a query row moves between key blocks and the accumulators are rescaled."""
    qkv, dout = make(FAM, ops, B, N, H, qk_mult=qk_mult)
    check_against_fp64(FAM, ops, qkv, dout, B, N, H)


@pytest.mark.parametrize("B,N,H", [(3, 1, 2), (3, 17, 2), (2, 197, 3), (1, 272, 2)])
def test_long_fp32_kernels_at_short_lengths_vs_fp64(ops, B, N, H):
    """The long kernels called directly where the whole-head kernels run: one row, a ragged single block, 197 and 272 tokens."""
    qkv, dout = make(FAM, ops, B, N, H, seed=5)
    check_against_fp64(FAM, ops, qkv, dout, B, N, H, long=True)


def test_long_fp32_attention_spiked_score(ops):
    """One query whose scores are ~30x the rest (scores of ~ +-300: one fp32 ulp of the score is 3e-5 in the exponent)."""
    B, N, H = 2, 577, 2
    qkv, dout = make(FAM, ops, B, N, H, seed=9)
    qkv = qkv.clone()
    qkv[0, 3, :FAM.dh] *= 30.0
    ref_in = qkv.double().requires_grad_(True)
    want, _ = attn_ref(ref_in, H, FAM.dh)
    want.backward(dout.double())
    out, lse = ops.attention_fwd_f32_lse(qkv.cuda(), B, N, H, FAM.scale)
    assert relerr(out, want) < FAM.bars["spike"]
    dqkv = ops.attention_bwd_f32_fused(qkv.cuda(), out, dout.cuda(), lse, B, N, H, FAM.scale)
    assert max(grad_errs(dqkv, ref_in.grad, B, N, H, FAM.dh)) < FAM.bars["spike"]


def test_short_lengths_keep_the_whole_head_fp32_kernels(ops):
    """At N <= 272 the wrappers call exactly what they called before: the whole-head kernels' bits."""
    check_short_lengths_keep_the_whole_head_kernels(FAM, ops, 2, 257, 2, seed=3)


def test_long_fp32_attention_key_permutation(ops):
    check_key_permutation(FAM, ops)


@pytest.mark.parametrize("N", [577, 1025])
def test_long_fp32_q8_codes_equal_quantised_output(ops, N):
    """The quantiser-fused forward of the converted int8 model: its codes are quant_affine_i8 of the plain output, bit for bit."""
    B, H = 2, 3
    qkv, _ = make(FAM, ops, B, N, H, seed=21)
    qkv_d = qkv.cuda()
    o = ops.attention_fwd_f32(qkv_d, B, N, H, FAM.scale)
    for s2, z2 in ((0.004, 131), (0.0125, 0), (0.002, 255)):
        codes = ops.attention_fwd_f32_q8(qkv_d, B, N, H, FAM.scale, s2, z2)
        assert torch.equal(codes.view(B * N, H * FAM.dh),
                           ops.quant_affine_i8(o.view(B * N, H * FAM.dh), B * N, H * FAM.dh, s2, z2))


def test_long_fp32_attention_keeps_no_n_squared_tensor(ops):
    """ViT-B heads at 1 025 tokens (512^2 segmentation), batch 8: attention_core forward + backward on fp32 q/k/v allocates less
    than half of one [B, H, N, N] fp32 tensor (403 MB); the materialised path holds the probabilities and a dP of that size."""
    check_no_n_squared_tensor(FAM, ops, 8, 12, 1025)


# ---------------------------------------------------------------- models
def test_fp32_model_at_384_never_materialises(ops):
    _, kw, params, img, labels = model_case(*CLS_384[:3], 2, CLS_384[3])
    with watching(ops, **WATCH["fp32"]):
        logits, grads = run_model(build_model(kw, "fp32", params), img, labels)
    assert bool(torch.isfinite(logits).all()) and len(grads) > 20


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("decoder,image_size,num_classes,name", MODEL_CASES)
def test_exact_modes_with_long_fp32_attention_match_oracle(ops, precision, decoder, image_size, num_classes, name):
    """fp32 and bf16x3 at the north-star contract, every block's attention on the key-tiled fp32 kernels (no fall-back)."""
    check_model_matches_oracle(FAM, ops, precision, decoder, image_size, num_classes, name)


@pytest.mark.parametrize("decoder,image_size,num_classes,name", MODEL_CASES)
def test_fp32_model_long_attention_vs_materialised(ops, decoder, image_size, num_classes, name):
    """The fp32 mode with ATTN_LONG off (materialised attention) and on (key-tiled) in one process: logits within mat_logits of
    max |logit|, every gradient tensor within mat_grad relative L2."""
    _, kw, params, img, labels = model_case(decoder, image_size, num_classes, 2, name)
    with watching(ops, attn_long=False):
        mat = run_model(build_model(kw, "fp32", params), img, labels)
    with watching(ops, **WATCH["fp32"]):
        long = run_model(build_model(kw, "fp32", params), img, labels)
    err, worst = assert_long_vs_materialised(FAM.bars, name, long, mat)
    report(f"attn_long_f32 fp32 {decoder} {image_size} logits long vs materialised", err)
    report(f"attn_long_f32 fp32 {decoder} {image_size} worst gradient long vs materialised", worst)


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
    assert np.isfinite(got).all() and err < INT8_MICRO_BAR, err
    top2 = np.sort(want, axis=1)[:, -2:]
    safe = (top2[:, 1] - top2[:, 0]) / scale > 2 * err
    assert (got.argmax(1) == want.argmax(1))[safe].all()


def test_graphed_fp32_step_equals_eager_step_at_384(ops):
    """577 tokens in fp32: the key-tiled fp32 kernels and their torch-allocated delta workspace inside the capture."""
    graphed_step_equals_eager(FAM.precision, 384)
