"""GPU: the key-tiled half-operand attention core of precision "bf16x3h" past 288 tokens (mv_attention_fwd_long_f16 / _bwd_long_f16).

The kernels against fp64 on the SAME half-rounded q/k/v through the dispatch and called directly at short lengths, at three
gradient magnitudes; the split-operand outputs and column sums; determinism; exact zeros; key-permutation invariance; the absence
of any [B, H, N, N] tensor; bf16x3h models at 384^2 and 512^2 against the CPU oracle at the precision's own bar and against the
fp32 mode; batch independence of ViT-B/16 at 384^2; graph capture.  Bars, builders and the bodies shared with the other families:
tests/attention_families.py (family "half")."""
import pytest
import torch

pytest.register_assert_rewrite("attention_families")   # its shared bodies assert: failures show the values
from attention_families import (CLS_384, FAMILIES, HALF_VS_FP32, SEG_512, VITB, build_model, check_against_fp64, check_deterministic,
                                check_key_permutation, check_model_matches_oracle, check_no_n_squared_tensor,
                                check_short_lengths_keep_the_whole_head_kernels, g, graphed_step_equals_eager, make, model_case, ops,
                                relerr, run_model, vit_b_384)  # noqa: F401

pytestmark = pytest.mark.gpu

FAM = FAMILIES["half"]
GSCALES = [1.0, 3.0e-7, 4.0e4]     # O(1), far below half's normal range, above half's largest value divided by the key count


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 289, 2, 1.0), (1, 300, 3, 1.0), (2, 321, 1, 1.0), (2, 577, 2, 1.0),
                                           (1, 577, 2, FAM.qk_mult), (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
@pytest.mark.parametrize("gscale", GSCALES)
def test_long_half_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult, gscale):
    """ops.attention_fwd_f16 / _bwd_f16 route N > 288 to the key-tiled half kernels.  qk_mult = 3: scores 9x larger, so the running
    maximum of a query row moves between key blocks and the accumulators are rescaled.  The same relative error at each gradient
    magnitude."""
    q16, dout = make(FAM, ops, B, N, H, gscale, qk_mult)
    check_against_fp64(FAM, ops, q16, dout, B, N, H)


@pytest.mark.parametrize("B,N,H", [(3, 1, 2), (3, 17, 2), (2, 64, 1), (2, 197, 3), (1, 257, 2)])
@pytest.mark.parametrize("gscale", GSCALES)
def test_long_half_kernels_at_short_lengths_vs_fp64(ops, B, N, H, gscale):
    """The long half kernels called directly where the whole-head kernels would run: one row, ragged blocks, exactly one block."""
    q16, dout = make(FAM, ops, B, N, H, gscale, seed=5)
    check_against_fp64(FAM, ops, q16, dout, B, N, H, long=True)


def test_short_lengths_keep_the_whole_head_half_kernels(ops):
    """N <= 288 still takes mv_attention_fwd_f16 / _bwd_f16: the dispatch gives exactly their bits, and they keep their cap."""
    check_short_lengths_keep_the_whole_head_kernels(FAM, ops, 2, 257, 3, seed=7)


def test_long_half_attention_is_deterministic(ops):
    check_deterministic(FAM, ops)


def test_long_half_attention_key_permutation(ops):
    check_key_permutation(FAM, ops)


def test_long_half_attention_keeps_no_n_squared_tensor(ops):
    """ViT-B heads at 1 025 tokens (512^2 segmentation), batch 8: neither the forward nor the backward (fp32 dqkv and its column
    sums) allocates anything near one [B, H, N, N] fp32 tensor (403 MB); the materialised path holds three."""
    check_no_n_squared_tensor(FAM, ops, 8, 12, 1025)


# ---------------------------------------------------------------- models
def test_bf16x3h_classification_384_matches_oracle(ops):
    check_model_matches_oracle(FAM, ops, "bf16x3h", *CLS_384)


def test_bf16x3h_segmentation_512_matches_oracle(ops):
    check_model_matches_oracle(FAM, ops, "bf16x3h", *SEG_512)


def test_bf16x3h_vs_fp32_full_tensors_at_384(ops):
    """Every element of every gradient tensor of bf16x3h against the fp32 mode, HALF_VS_FP32 relative L2 per tensor and on the
    logits: test_vit_parity.py's bf16x3h_vs_fp32_full_tensors at 384^2."""
    _, kw, params, img, labels = model_case(*CLS_384[:3], 2, CLS_384[3])
    l32, g32 = run_model(build_model(kw, "fp32", params), img, labels)
    lh, gh = run_model(build_model(kw, "bf16x3h", params), img, labels)
    assert float((lh - l32).abs().max() / l32.abs().max()) < HALF_VS_FP32
    assert set(gh) == set(g32) and len(g32) > 20
    for k, ref in g32.items():
        e = relerr(gh[k], ref)
        assert e < HALF_VS_FP32, (k, e)


def test_vit_b_384_bf16x3h_logits_are_per_sample_independent(ops):
    vit = vit_b_384("bf16x3h")
    img = torch.randn(64, 3, 384, 384, generator=g(11)).cuda()
    with torch.no_grad():
        full = vit(img).float()
        part = vit(img[40:48].contiguous()).float()
    assert relerr(full[40:48], part) < VITB["half_sample"]
    assert float((full[40:48] - part).abs().max() / part.abs().max()) < VITB["half_sample"]


def test_graphed_bf16x3h_step_equals_eager_step_at_384(ops):
    """577 tokens in bf16x3h: the long half kernels, their torch-allocated prep outputs and column-sum workspace inside the capture."""
    graphed_step_equals_eager(FAM.precision, 384)
