"""CPU: which lengths the exact-fp32 attention core of precisions "fp32" / "bf16x3" (and the converted int8 model) takes (the
key-tiled f32 kernels above 272 tokens), the A/B switch, and the three long fp32 entry points' argument checks."""
import pytest
import torch

MV_OK, MV_ERR_SHAPE, MV_ERR_ALIGN, MV_ERR_UNSUPPORTED = 0, -1, -2, -4      # include/myrtle_vision_hip.h


@pytest.fixture
def ops(monkeypatch):
    from myrtle_vision.hip import ops as _ops
    monkeypatch.setattr(_ops, "ATTN_LONG", True)
    return _ops


@pytest.mark.parametrize("N", [1, 197, 272, 273, 577, 1025, 4097, 8192])
def test_fp32_attention_is_fused_up_to_the_cap(ops, N):
    assert ops.attention_f32_fused_supported(torch.float32, N, 64)


def test_fp32_attention_limits(ops, monkeypatch):
    assert not ops.attention_f32_fused_supported(torch.float32, 8193, 64)
    assert not ops.attention_f32_fused_supported(torch.float32, 577, 32)
    assert not ops.attention_f32_fused_supported(torch.bfloat16, 577, 64)
    monkeypatch.setattr(ops, "ATTN_LONG", False)                         # the A/B tool's materialised arm
    assert ops.attention_f32_fused_supported(torch.float32, 272, 64)
    assert not ops.attention_f32_fused_supported(torch.float32, 273, 64)
    assert not ops.attention_f32_fused_supported(torch.float32, 577, 64)


def test_bf16_and_half_dispatch_is_unchanged(ops, monkeypatch):
    assert ops.attention_fused_supported(torch.bfloat16, 577, 64) and not ops.attention_fused_supported(torch.float32, 577, 64)
    with ops.segments(4):
        assert ops.attention_f16_supported(torch.float32, 577, 64)
    for nseg in (3, 6):
        with ops.segments(nseg):
            assert not ops.attention_f16_supported(torch.float32, 577, 64)
    monkeypatch.setattr(ops, "ATTN_LONG", False)
    assert ops.attention_fused_supported(torch.bfloat16, 320, 64) and not ops.attention_fused_supported(torch.bfloat16, 321, 64)
    with ops.segments(4):
        assert ops.attention_f16_supported(torch.float32, 288, 64) and not ops.attention_f16_supported(torch.float32, 289, 64)


def test_long_fp32_entry_points_are_bound():
    from myrtle_vision.hip import lib
    handle = lib.lib()
    assert lib.SIGNATURES["mv_attention_fwd_long_f32"][0] == "ppp" "iii" "f" "p"
    assert lib.SIGNATURES["mv_attention_fwd_long_f32_q8"][0] == "pp" "iii" "f" "f" "i" "p"
    assert lib.SIGNATURES["mv_attention_bwd_long_f32"][0] == "pppppp" "iii" "f" "p"
    for name in ("mv_attention_fwd_long_f32", "mv_attention_fwd_long_f32_q8", "mv_attention_bwd_long_f32"):
        assert getattr(handle, name) is not None


def test_long_fp32_entry_points_reject_bad_arguments():
    """Argument checks run before any device work: lengths past the cap, a bad quantiser, misaligned pointers and a missing lse or
    delta workspace."""
    from myrtle_vision.hip import lib
    L = lib.lib()
    a = 1 << 20                                       # a 16-byte-aligned address that is never dereferenced (rejected first)
    fwd, q8, bwd = L.mv_attention_fwd_long_f32, L.mv_attention_fwd_long_f32_q8, L.mv_attention_bwd_long_f32
    assert fwd(a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert fwd(a, a, None, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert fwd(a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert fwd(a, a, a, -1, 577, 1, 0.125, None) == MV_ERR_SHAPE
    assert fwd(a + 4, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert fwd(a, a + 8, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert q8(a, a, 1, 8193, 1, 0.125, 0.05, 128, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.05, 256, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.05, -1, None) == MV_ERR_UNSUPPORTED
    assert q8(a, a, 1, 577, 1, 0.125, 0.0, 128, None) == MV_ERR_SHAPE
    assert q8(a, a + 2, 1, 577, 1, 0.125, 0.05, 128, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert bwd(a, a, a, a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert bwd(a, a + 4, a, a, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a + 4, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, None, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN            # no lse
    assert bwd(a, a, a, a, None, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN            # no delta workspace
    # B = 0 is a no-op that launches nothing
    assert fwd(a, a, a, 0, 577, 1, 0.125, None) == MV_OK
    assert fwd(a, a, None, 0, 577, 1, 0.125, None) == MV_OK
    assert q8(a, a, 0, 577, 1, 0.125, 0.05, 128, None) == MV_OK
    assert bwd(a, a, a, a, a, a, 0, 577, 1, 0.125, None) == MV_OK
