"""GPU: the key-tiled bf16 attention core for sequences longer than 320 tokens (mv_attention_fwd_long / _bwd_long).

ViT-B/16 at 384^2 has 577 tokens, patch 8 at 224^2 785, segmentation at 512^2 1 025: the whole-head kernels stop at 320.  The
kernels against fp64, the long kernels at short lengths, determinism, key-permutation invariance, the absence of any [B, H, N, N]
tensor, whole models against the CPU oracle at the bf16 envelope, graph capture, and the batch-decomposition properties of
ViT-B/16 at 384^2.  Bars, builders and the bodies shared with the other families: tests/attention_families.py (family "bf16")."""
import pytest
import torch

pytest.register_assert_rewrite("attention_families")   # its shared bodies assert: failures show the values
from attention_families import (CLS_384, FAMILIES, SEG_512, VITB, check_against_fp64, check_deterministic, check_key_permutation,
                                check_model_matches_oracle, check_no_n_squared_tensor, check_short_lengths_keep_the_whole_head_kernels,
                                g, graphed_step_equals_eager, make, ops, rel_l2, vit_b_384)  # noqa: F401

pytestmark = pytest.mark.gpu

FAM = FAMILIES["bf16"]


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("B,N,H,qk_mult", [(2, 321, 2, 1.0), (1, 385, 3, 1.0), (2, 577, 2, 1.0), (1, 577, 2, FAM.qk_mult),
                                           (1, 785, 2, 1.0), (1, 1025, 2, 1.0), (1, 4097, 1, 1.0)])
def test_long_attention_through_the_dispatch_vs_fp64(ops, B, N, H, qk_mult):
    """ops.attention_fwd / _bwd route N > 320 to the key-tiled kernels.  qk_mult = 4: scores 16x larger, so the running maximum
    of a query row really moves between key blocks and the accumulators are rescaled."""
    qkv, dout = make(FAM, ops, B, N, H, qk_mult=qk_mult)
    check_against_fp64(FAM, ops, qkv, dout, B, N, H)


@pytest.mark.parametrize("B,N,H", [(3, 17, 2), (2, 197, 3), (1, 257, 2), (2, 320, 1)])
def test_long_kernels_at_short_lengths_vs_fp64(ops, B, N, H):
    qkv, dout = make(FAM, ops, B, N, H, seed=5)
    check_against_fp64(FAM, ops, qkv, dout, B, N, H, long=True)


def test_short_lengths_keep_the_whole_head_kernels(ops):
    """N <= 320 still takes mv_attention_fwd / _bwd: ops.attention_fwd gives exactly their bits."""
    check_short_lengths_keep_the_whole_head_kernels(FAM, ops, 2, 197, 3, seed=7)


def test_long_attention_is_deterministic(ops):
    check_deterministic(FAM, ops)


def test_long_attention_key_permutation(ops):
    check_key_permutation(FAM, ops)


def test_attention_core_keeps_no_n_squared_tensor(ops):
    check_no_n_squared_tensor(FAM, ops, 8, 12, 1025)


# ---------------------------------------------------------------- models
def test_bf16_classification_384_matches_oracle(ops):
    check_model_matches_oracle(FAM, ops, "bf16", *CLS_384)


def test_bf16_segmentation_512_matches_oracle(ops):
    check_model_matches_oracle(FAM, ops, "bf16", *SEG_512)


def test_graphed_step_equals_eager_step_at_384(ops):
    """577 tokens: the key-tiled kernels and their torch-allocated delta workspace inside the capture."""
    graphed_step_equals_eager(FAM.precision, 384)


# ---------------------------------------------------------------- ViT-B/16 at 384^2, batch 64
@pytest.fixture(scope="module")
def vit_b384():
    return vit_b_384("bf16")


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
    assert rel_l2(full[40:48], part) < VITB["bf16_sample"]
    assert torch.equal(full[40:48].argmax(1), part.argmax(1))


def test_vit_b_384_gradient_is_the_mean_of_its_halves(vit_b384):
    img = torch.randn(64, 3, 384, 384, generator=g(12)).cuda()
    labels = torch.randint(0, 1000, (64,), generator=g(13)).cuda()
    loss, full = _grads(vit_b384, img, labels)
    l0, h0 = _grads(vit_b384, img[:32].contiguous(), labels[:32].contiguous())
    l1, h1 = _grads(vit_b384, img[32:].contiguous(), labels[32:].contiguous())
    assert abs(loss - 0.5 * (l0 + l1)) < VITB["loss_halves"] * abs(loss)
    assert set(full) == set(h0) == set(h1) and len(full) > 140
    worst = max(rel_l2(0.5 * (h0[n] + h1[n]), full[n]) for n in full)
    assert worst < VITB["grad_halves"], worst
