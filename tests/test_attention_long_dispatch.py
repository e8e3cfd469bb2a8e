"""CPU: which bf16 attention lengths take the fused kernels (the key-tiled ones above 320 tokens), and the A/B switch."""
import pytest
import torch


@pytest.fixture
def ops(monkeypatch):
    from myrtle_vision.hip import ops as _ops
    monkeypatch.setattr(_ops, "ATTN_LONG", True)
    return _ops


@pytest.mark.parametrize("N", [1, 197, 257, 320, 321, 577, 785, 1025, 4097, 8192])
def test_bf16_attention_is_fused_up_to_the_cap(ops, N):
    assert ops.attention_fused_supported(torch.bfloat16, N, 64)


def test_fused_attention_limits(ops, monkeypatch):
    assert not ops.attention_fused_supported(torch.bfloat16, 8193, 64)
    assert not ops.attention_fused_supported(torch.bfloat16, 577, 32)
    assert not ops.attention_fused_supported(torch.float32, 577, 64)      # fp32 / bf16x3 / bf16x3h keep their paths
    monkeypatch.setattr(ops, "ATTN_LONG", False)                            # the A/B tool's materialised arm
    assert ops.attention_fused_supported(torch.bfloat16, 320, 64)
    assert not ops.attention_fused_supported(torch.bfloat16, 321, 64)


def test_long_entry_points_are_bound():
    from myrtle_vision.hip import lib
    handle = lib.lib()
    assert lib.SIGNATURES["mv_attention_bwd_long"][0] == "ppppppp" "iii" "f" "p"
    assert handle.mv_attention_fwd_long is not None and handle.mv_attention_bwd_long is not None
