"""CPU: which lengths the half-operand attention core of precision "bf16x3h" takes (the key-tiled half kernels above 288 tokens),
the A/B switch, and the two long half entry points."""
import pytest
import torch

MV_OK, MV_ERR_SHAPE, MV_ERR_ALIGN, MV_ERR_UNSUPPORTED = 0, -1, -2, -4      # include/myrtle_vision_hip.h


@pytest.fixture
def ops(monkeypatch):
    from myrtle_vision.hip import ops as _ops
    monkeypatch.setattr(_ops, "ATTN_LONG", True)
    return _ops


@pytest.mark.parametrize("N", [1, 197, 257, 288, 289, 321, 577, 1025, 4097, 8192])
def test_half_attention_is_fused_up_to_the_cap(ops, N):
    with ops.segments(4):
        assert ops.attention_f16_supported(torch.float32, N, 64)


def test_half_attention_limits(ops, monkeypatch):
    with ops.segments(4):
        assert not ops.attention_f16_supported(torch.float32, 8193, 64)
        assert not ops.attention_f16_supported(torch.float32, 577, 32)
        assert not ops.attention_f16_supported(torch.bfloat16, 577, 64)
        monkeypatch.setattr(ops, "ATTN_LONG", False)                         # the A/B tool's materialised arm
        assert ops.attention_f16_supported(torch.float32, 288, 64)
        assert not ops.attention_f16_supported(torch.float32, 289, 64)
        assert not ops.attention_f16_supported(torch.float32, 577, 64)
    monkeypatch.setattr(ops, "ATTN_LONG", True)
    for nseg in (3, 6):                                                         # outside the half-attention scope
        with ops.segments(nseg):
            assert not ops.attention_f16_supported(torch.float32, 577, 64)
            assert not ops.attention_f16_supported(torch.float32, 197, 64)


def test_fused_bf16_dispatch_is_unchanged(ops):
    assert not ops.attention_fused_supported(torch.float32, 577, 64)
    with ops.segments(4):
        assert not ops.attention_fused_supported(torch.float32, 577, 64)


def test_long_half_entry_points_are_bound():
    from myrtle_vision.hip import lib
    handle = lib.lib()
    assert lib.SIGNATURES["mv_attention_fwd_long_f16"][0] == "ppp" "iii" "f" "p"
    assert lib.SIGNATURES["mv_attention_bwd_long_f16"][0] == "pppppp" "ipp" "iii" "f" "p"
    assert handle.mv_attention_fwd_long_f16 is not None and handle.mv_attention_bwd_long_f16 is not None


def test_long_half_entry_points_reject_bad_arguments():
    """Argument checks run before any device work: shapes past the cap, a bad segment count and misaligned or missing pointers."""
    from myrtle_vision.hip import lib
    L = lib.lib()
    a = 1 << 20                                       # a 16-byte-aligned address that is never dereferenced (rejected first)
    assert L.mv_attention_fwd_long_f16(a, a, a, 1, 8193, 1, 0.125, None) == MV_ERR_SHAPE
    assert L.mv_attention_fwd_long_f16(a, a, a, 1, 0, 1, 0.125, None) == MV_ERR_SHAPE
    assert L.mv_attention_fwd_long_f16(a + 2, a, a, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    bwd = L.mv_attention_bwd_long_f16
    assert bwd(a, a, a, a, a, a, 0, None, None, 1, 8193, 1, 0.125, None) == MV_ERR_SHAPE
    assert bwd(a, a, a, a, a, a, 4, None, None, 1, 577, 1, 0.125, None) == MV_ERR_UNSUPPORTED
    assert bwd(a, a + 8, a, a, a, a, 3, None, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN
    assert bwd(a, a, a, a, a, a, 6, a, None, 1, 577, 1, 0.125, None) == MV_ERR_ALIGN      # colsum without its workspace
    # B = 0 is a no-op that launches nothing
    assert L.mv_attention_fwd_long_f16(a, a, a, 0, 577, 1, 0.125, None) == MV_OK
    assert bwd(a, a, a, a, a, a, 0, a, a, 0, 577, 1, 0.125, None) == MV_OK
