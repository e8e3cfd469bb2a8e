"""CPU: which head widths other than 64 take fused bf16 attention kernels (32 and 128, mv_attention_fwd_dh / _bwd_dh), the A/B
switch, the bindings, and the branch functional.attention_core takes for them."""
import pytest
import torch


@pytest.fixture
def ops(monkeypatch):
    from myrtle_vision.hip import ops as _ops
    monkeypatch.setattr(_ops, "ATTN_LONG", True)
    return _ops


@pytest.mark.parametrize("w", [32, 128])
@pytest.mark.parametrize("N", [1, 197, 321, 577, 8192])
def test_widths_32_and_128_are_fused_at_every_length(ops, N, w):
    assert ops.ATTN_DH_WIDTHS == (32, 128)
    assert ops.attention_dh_supported(torch.bfloat16, N, w)


def test_dh_limits_and_the_ab_switch(ops, monkeypatch):
    for w in (32, 128):
        assert not ops.attention_dh_supported(torch.bfloat16, 8193, w)
        assert not ops.attention_dh_supported(torch.float32, 577, w)         # fp32-qkv modes keep the materialised path
    for w in (48, 64, 96):
        assert not ops.attention_dh_supported(torch.bfloat16, 577, w)        # 64 has kernels of its own
    monkeypatch.setattr(ops, "ATTN_LONG", False)                             # the A/B tools' materialised arm
    for w in (32, 48, 64, 96, 128):
        for N in (1, 197, 321, 577, 8192):
            assert not ops.attention_dh_supported(torch.bfloat16, N, w)


@pytest.mark.parametrize("long_on", [True, False])
def test_the_64_wide_predicates_keep_their_meaning(ops, monkeypatch, long_on):
    monkeypatch.setattr(ops, "ATTN_LONG", long_on)
    monkeypatch.setattr(ops, "half_attention", lambda: True)
    for w in (32, 128):
        for N in (1, 197, 577):
            assert not ops.attention_fused_supported(torch.bfloat16, N, w)
            assert not ops.attention_f32_fused_supported(torch.float32, N, w)
            assert not ops.attention_f16_supported(torch.float32, N, w)
    assert ops.attention_fused_supported(torch.bfloat16, 197, 64)


def test_dh_entry_points_are_bound():
    from myrtle_vision.hip import lib
    handle = lib.lib()
    assert lib.SIGNATURES["mv_attention_fwd_dh"][0] == "ppp" "iiii" "f" "p"
    assert lib.SIGNATURES["mv_attention_bwd_dh"][0] == "ppppppp" "iiii" "f" "p"
    assert handle.mv_attention_fwd_dh is not None and handle.mv_attention_bwd_dh is not None


class _Materialised(Exception):
    pass


@pytest.fixture
def recorded(ops, monkeypatch):
    """ops.attention_fwd_dh / _bwd_dh replaced by recorders that return tensors of the right shapes (no device needed); the first
    step of the materialised path (the cast of qkv to fp32) raises ``_Materialised``."""
    from myrtle_vision.hip import functional as F
    calls = []

    def fwd(qkv, B, N, H, dh, scale):
        calls.append(("fwd", B, N, H, dh))
        return torch.zeros(B, N, H * dh, dtype=torch.bfloat16), torch.zeros(B, H, N)

    def bwd(qkv, out, dout, lse, B, N, H, dh, scale, colsum=None):
        calls.append(("bwd", B, N, H, dh))
        assert dout.dtype == torch.bfloat16 and colsum is None
        return torch.ones_like(qkv)

    def no_cast(*a, **k):
        raise _Materialised()

    monkeypatch.setattr(ops, "attention_fwd_dh", fwd)
    monkeypatch.setattr(ops, "attention_bwd_dh", bwd)
    monkeypatch.setattr(F, "cast", no_cast)
    return F, calls


@pytest.mark.parametrize("dh", [32, 128])
def test_attention_core_takes_the_dh_branch(recorded, dh):
    F, calls = recorded
    B, N, H = 2, 197, 3
    qkv = torch.zeros(B, N, 3 * H * dh, dtype=torch.bfloat16, requires_grad=True)
    out = F.attention_core(qkv, H, dh ** -0.5)
    assert out.shape == (B, N, H * dh) and calls == [("fwd", B, N, H, dh)]
    out.backward(torch.ones_like(out))
    assert calls == [("fwd", B, N, H, dh), ("bwd", B, N, H, dh)]
    assert qkv.grad is not None and bool((qkv.grad == 1).all())


@pytest.mark.parametrize("dh", [32, 128])
def test_attention_core_with_a_hook_keeps_the_materialised_path(recorded, dh):
    F, calls = recorded
    qkv = torch.zeros(2, 197, 3 * 3 * dh, dtype=torch.bfloat16)
    with pytest.raises(_Materialised):
        F.attention_core(qkv, 3, dh ** -0.5, probs_hook=lambda p: p)
    assert calls == []


@pytest.mark.parametrize("case", [("bf16", 48), ("fp32", 32), ("off", 128)])
def test_attention_core_leaves_other_cases_on_the_materialised_path(recorded, ops, monkeypatch, case):
    F, calls = recorded
    kind, dh = case
    if kind == "off":
        monkeypatch.setattr(ops, "ATTN_LONG", False)
    qkv = torch.zeros(2, 197, 3 * 3 * dh, dtype=torch.float32 if kind == "fp32" else torch.bfloat16, requires_grad=True)
    with pytest.raises(_Materialised):
        F.attention_core(qkv, 3, dh ** -0.5)
    assert calls == []
