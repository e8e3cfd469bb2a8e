"""GPU: the fused attention block (``functional.attn_block``) on every attention path, forward and backward, against the same block
assembled from the granular functions (``layer_norm`` / ``linear`` / ``attention_core`` / ``linear`` + residual add).  Both sides
launch the same attention kernels on the same q/k/v, so whatever the two compositions share is compared bit for bit; see
``EXACT`` for what they share on each path and ``CLOSE`` for the rest."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, H = 2, 2
NAMES = ("out", "dx", "dg", "db", "dwqkv", "dbqkv", "dwo", "dbo")


def block_and_granular(prec, dh, N, grad=True, seed=0, B=B):
    """-> ({name: tensor} of the fused block, the same of the granular composition, the input x), from identical inputs."""
    from myrtle_vision.hip import functional as F
    from myrtle_vision.hip import ops
    D = H * dh
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).cuda()
    base = [rnd(B, N, D), 1 + rnd(D, scale=0.1), rnd(D, scale=0.1), rnd(3 * D, D, scale=D ** -0.5), rnd(3 * D, scale=0.1),
            rnd(D, D, scale=D ** -0.5), rnd(D, scale=0.1)]
    dout = rnd(B, N, D)
    adt, scale = ops.act_dtype(prec), dh ** -0.5

    def fused(x, g, b, wqkv, bqkv, wo, bo):
        F.chain_reset()
        return F.attn_block(x, g, b, wqkv, bqkv, wo, bo, H, scale, prec)

    def granular(x, g, b, wqkv, bqkv, wo, bo):
        with ops.segments(ops.prec_segments(prec)):
            qkv = F.linear(F.layer_norm(x, g, b, adt), wqkv, bqkv)
            return F.add(F.linear(F.attention_core(qkv, H, scale), wo, bo), x)

    res = []
    for fn in (fused, granular):
        args = [t.clone().requires_grad_(grad) for t in base]
        out = fn(*args)
        assert out.requires_grad == grad
        if grad:
            out.backward(dout)
        torch.cuda.synchronize()
        res.append(dict(zip(NAMES, [out.detach()] + [a.grad for a in args])) if grad else {"out": out.detach()})
    return res[0], res[1], base[0]


def relerr(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm().clamp_min(1e-30))


def relmax(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max().clamp_min(1e-30))


# What the two compositions do NOT share, per case; every other output and gradient must be torch.equal (measured so on the
# commit before the routing went through ops.attention_path, and unchanged by it):
# The figures in brackets are the largest this test's cases gave on that commit (and give now: the two trees agree bit for bit).
#   "proj16"  bf16: the granular projection leaves as bf16 and the residual is added by a second kernel; the block's GEMM epilogue
#             adds bias and residual to the fp32 accumulator.  One bf16 rounding of the projection p (bf16 carries 8 significant
#             bits: unit roundoff 2^-8, |round(p) - p| <= 2^-8 |p| <= 2^-8 (1 + 2^-7) |round(p)|) and the fp32 roundings of the
#             two sums: |d out| <= 2^-8 (1 + 2^-7) |out_granular - x| + 2^-22 max |out|, element by element.  [0.987 of it]
#   "proj32"  the split-operand branch (B * N >= 128): the same with fp32 roundings only: max |d out| <= 2^-22 max |out|.  [1.13e-7 = 2^-23.1]
#   "colsum"  to_qkv's bias gradient from the attention kernel's column sums (fp32 sums of the accumulators, before dqkv is
#             rounded to bf16) against the dW pass's sums of the rounded dqkv: the bar of tests/test_attention_short.py, 5e-3 of max.  [4.6e-4]
#   "half"    precision "bf16x3h" in the split-operand branch: the block runs the half-operand kernels, attention_core never
#             does (it runs the exact fp32 ones), so everything downstream of the core is only as close as the precision's
#             contract: 1e-3 relative in norm, the bar of tests/test_vit_parity.py and smoke() for this precision.  [4.7e-4]
CASES = [           # precision, dh, N, gradients, what is only close, batch (2 unless given)
    ("bf16", 64, 17, True, ("proj16", "colsum")),            # whole-head kernels
    ("bf16", 64, 321, True, ("proj16", "colsum")),           # the first key-tiled length
    ("bf16", 32, 17, True, ("proj16", "colsum")),
    ("bf16", 128, 17, True, ("proj16", "colsum")),
    ("bf16", 48, 17, True, ("proj16",)),                     # no fused kernel: materialised probabilities
    ("bf16x3h", 64, 17, True, ()),                           # 34 rows: the plain fp32 branch, exact fp32 core on both sides
    ("bf16x3h", 64, 17, True, ("half",), 8),                 # 136 rows: the split-operand branch, whole-head half kernels
    ("bf16x3h", 64, 289, True, ("half",)),                   # the first key-tiled half length
    ("fp32", 64, 17, True, ()),                              # the plain fp32 branch, whole-head fp32 kernels
    ("fp32", 64, 17, False, ()),
    ("fp32", 64, 17, True, ("proj32",), 8),                  # the split-operand branch, whole-head fp32 kernels
    ("fp32", 64, 17, False, ("proj32",), 8),
    ("fp32", 64, 273, True, ("proj32",)),                    # the first key-tiled fp32 length
    ("fp32", 64, 273, False, ("proj32",)),
]


def case_id(c):
    return f"{c[0]}-dh{c[1]}-N{c[2]}-{'grad' if c[3] else 'eval'}" + (f"-B{c[5]}" if len(c) > 5 else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_attn_block_matches_the_granular_composition(case):
    prec, dh, N, grad, close = case[:5]
    blk, gran, x = block_and_granular(prec, dh, N, grad, B=case[5] if len(case) > 5 else B)
    assert set(blk) == set(gran) == (set(NAMES) if grad else {"out"})
    for name in blk:
        got, want = blk[name], gran[name]
        assert got.shape == want.shape and got.dtype == want.dtype == torch.float32 and bool(torch.isfinite(got).all()), name
        how = "equal"
        if "half" in close and name != "dbo":                # dbo is the column sum of dout on both sides
            how = f"half {relerr(got, want):.2e}"
            ok = relerr(got, want) < 1e-3
        elif name == "out" and "proj16" in close:
            bar = 2.0 ** -8 * (1 + 2.0 ** -7) * (want - x).abs() + 2.0 ** -22 * want.abs().max()
            how = f"proj16 {float(((got - want).abs() / bar).max()):.2f} of the bar"
            ok = bool(((got - want).abs() <= bar).all())
        elif name == "out" and "proj32" in close:
            how = f"proj32 {relmax(got, want):.2e}"
            ok = relmax(got, want) <= 2.0 ** -22
        elif name == "dbqkv" and "colsum" in close:
            how = f"colsum {relmax(got, want):.2e}"
            ok = relmax(got, want) < 5e-3
        else:
            ok = torch.equal(got, want)
        print(f"{prec} dh{dh} N{N} {name}: {how}")
        assert ok, (name, how)
