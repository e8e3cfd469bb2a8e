"""One ViT-B block (attn_block -> mlp_block, dim 768, bf16) forward and backward with the to_out / to_qkv weight gradients in one
grouped split-K launch and with the grouping switched off (TN force code + 1000).

Only the two weight gradients may differ, and only by fp32 summation order (the split count changes); everything else -- dx, the
LayerNorm and bias gradients, the MLP block's gradients -- must be bit-equal: the grouped launch reads the same operands and
nothing downstream reads dW.

* 2 x 197 tokens = 394 rows: no multiple of 32, so the library runs the two products one by one whatever the force code says:
  every gradient bit-equal.
* 32 x 64 tokens = 2048 rows.  The automatic dispatch keeps the 256-tile kernel (and with it the grouping) for contractions of
  4096 rows and more, so at family 0 this is the one-by-one path again: every gradient bit-equal.  With the 256-tile kernel forced
  (256 against 1256) the pair really shares a launch: 36 tiles -> 4 splits of 16 stages, where the products alone run 9 tiles -> 4
  splits and 27 tiles -> 4 splits -- the same split boundaries -- so here even the sums agree bit for bit, and the bar below (the
  bf16 dW bar of tests/test_hip_ops.py, 3e-6 of the largest element) holds trivially.
* 32 x 160 tokens = 5120 rows, 256-tile kernel forced: 36 tiles -> 7 splits against 10 (9 tiles) and 9 (27 tiles): the summation
  order differs, the bar is what holds."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, HD = 768, 12, 3072
DW_BAR = 3e-6                # tests/test_hip_ops.py: test_gemm_tn_dw_and_colsum, test_gemm_tn_every_variant
PAIRED = ("wqkv", "wo")


def g(seed):
    return torch.Generator().manual_seed(seed)


def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


@pytest.fixture(scope="module")
def params():
    p = {"g1": torch.randn(D, generator=g(20)) * 0.1 + 1, "b1": torch.randn(D, generator=g(21)) * 0.1,
         "wqkv": torch.randn(3 * D, D, generator=g(22)) * D ** -0.5, "bqkv": torch.randn(3 * D, generator=g(23)) * 0.1,
         "wo": torch.randn(D, D, generator=g(24)) * D ** -0.5, "bo": torch.randn(D, generator=g(25)) * 0.1,
         "g2": torch.randn(D, generator=g(26)) * 0.1 + 1, "b2": torch.randn(D, generator=g(27)) * 0.1,
         "w1": torch.randn(HD, D, generator=g(28)) * D ** -0.5, "bf1": torch.randn(HD, generator=g(29)) * 0.1,
         "w2": torch.randn(D, HD, generator=g(30)) * HD ** -0.5, "bf2": torch.randn(D, generator=g(31)) * 0.1}
    return {k: v.cuda() for k, v in p.items()}


def block_grads(params, B, T, force):
    from myrtle_vision.hip import functional as F
    from myrtle_vision.hip.lib import check, lib
    x = torch.randn(B, T, D, generator=g(32)).cuda().requires_grad_(True)
    r = torch.randn(B, T, D, generator=g(33)).cuda()
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    check(lib().mv_gemm_force_variant(0, force), "force_variant")
    try:
        F.chain_reset()
        h = F.attn_block(x, ps["g1"], ps["b1"], ps["wqkv"], ps["bqkv"], ps["wo"], ps["bo"], H, (D // H) ** -0.5, "bf16")
        out = F.mlp_block(h, ps["g2"], ps["b2"], ps["w1"], ps["bf1"], ps["w2"], ps["bf2"], "bf16")
        (out * r).sum().backward()
        torch.cuda.synchronize()
    finally:
        check(lib().mv_gemm_force_variant(0, 0), "force_variant")
    grads = {k: v.grad for k, v in ps.items()}
    grads["x"] = x.grad
    grads["out"] = out.detach()
    return grads


@pytest.mark.parametrize("B,T,family,same_sums", [(2, 197, 0, True), (2, 197, 256, True), (32, 64, 0, True), (32, 64, 256, True),
                                                  (32, 160, 256, False)])
def test_block_gradients_with_grouping_on_and_off(params, B, T, family, same_sums):
    on = block_grads(params, B, T, family)
    off = block_grads(params, B, T, family + 1000)
    for name in on:
        assert on[name] is not None and torch.isfinite(on[name]).all(), name
        if name in PAIRED:
            err = relerr(on[name], off[name])
            print(f"{name}: grouped against single, max difference / max element = {err:.3e}")
            assert err < DW_BAR, name
            if same_sums:
                assert torch.equal(on[name], off[name]), name
        else:
            assert torch.equal(on[name], off[name]), name
    if not same_sums:        # 7 slabs against 10 and 9: equal bits here would mean the grouped launch never ran
        assert not torch.equal(on["wo"], off["wo"]) and not torch.equal(on["wqkv"], off["wqkv"])
    again = block_grads(params, B, T, family)
    for name in PAIRED:
        assert torch.equal(on[name], again[name]), name
