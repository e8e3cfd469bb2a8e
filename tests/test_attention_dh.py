"""GPU: the fused bf16 attention core for 32- and 128-wide heads (mv_attention_fwd_dh / _bwd_dh), any N up to 8 192.

The kernels against fp64 from the same bf16 inputs at the bars of the 64-wide key-tiled kernels (same rounding points: P and dS
rounded to bf16, fp32 accumulation, outputs rounded once), determinism, the rejections of the C entry points, the absence of any
[B, H, N, N] tensor, and whole models of both widths against the CPU oracle at the bf16 envelope and against the materialised
path (``ops.ATTN_LONG`` off: what these widths took before).  Bars, builders and the bodies shared with the other families:
tests/attention_families.py (families "dh32" and "dh128")."""
import pytest
import torch

pytest.register_assert_rewrite("attention_families")   # its shared bodies assert: failures show the values
from attention_families import (FAMILIES, check_against_fp64, check_deterministic, check_model_matches_oracle,
                                check_no_n_squared_tensor, make, ops)  # noqa: F401
from test_attention_short import MV_ERR_ALIGN, MV_ERR_SHAPE, MV_ERR_UNSUPPORTED

pytestmark = pytest.mark.gpu

WIDTHS = [32, 128]


def fam_of(dh):
    return FAMILIES[f"dh{dh}"]


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("dh", WIDTHS)
@pytest.mark.parametrize("B,N,H", [(2, 1, 2), (3, 15, 2), (2, 64, 3), (2, 65, 2), (2, 197, 3), (1, 257, 2), (2, 577, 2),
                                   (1, 1025, 2), (1, 4097, 1)])
def test_dh_attention_vs_fp64(ops, B, N, H, dh):
    qkv, dout = make(fam_of(dh), ops, B, N, H, seed=3 + N)
    check_against_fp64(fam_of(dh), ops, qkv, dout, B, N, H)


@pytest.mark.parametrize("dh", WIDTHS)
def test_dh_attention_vs_fp64_with_moving_maxima(ops, dh):
    """q and k four times larger: scores 16x larger, so the running maximum of a query row really moves between key blocks and
    the accumulators are rescaled."""
    fam = fam_of(dh)
    qkv, dout = make(fam, ops, 1, 577, 2, qk_mult=fam.qk_mult, seed=23)
    check_against_fp64(fam, ops, qkv, dout, 1, 577, 2)


@pytest.mark.parametrize("dh", WIDTHS)
def test_dh_attention_is_deterministic(ops, dh):
    check_deterministic(fam_of(dh), ops)


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
    check_no_n_squared_tensor(fam_of(dh), ops, 8, 26, 577)


# ---------------------------------------------------------------- models
@pytest.mark.parametrize("dh", WIDTHS)
@pytest.mark.parametrize("decoder,image_size,num_classes", [("classification", 224, 45), ("segmentation", 384, 17)])
def test_bf16_model_matches_oracle_and_materialised_path(ops, decoder, image_size, num_classes, dh):
    check_model_matches_oracle(fam_of(dh), ops, "bf16", decoder, image_size, num_classes, f"dh{dh}_{decoder}_{image_size}")
