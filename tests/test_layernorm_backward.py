"""GPU: LayerNorm backward (mv_layernorm_bwd / mv_layernorm_bwd_split) in every form the model calls it, against fp64 autograd
through oracle.vit_oracle.layer_norm, plus the bitwise identities its fused by-products promise -- and the hand-off of those
by-products from one fused transformer block's backward to the block before it.

Forms:  (a) plain (+ dx_add);  (b) the bf16 step's: dx16 (bf16 copy of dx) + dx_colsum;  (c) the split-operand modes': the bf16
pieces of dx (nseg 3 / 6) + dx_colsum;  (d) dx_colsum alone;  (e) the classification head's: cls rows T*D apart, no dx_add.
Row counts above 4 096 run the grid-stride loop (the grid is capped at 1 024 blocks of 4 waves), where every wave accumulates its
dgamma / dbeta / colsum partials over several rows.  Tolerances are written next to each check."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.vit_oracle import layer_norm as ln_oracle  # noqa: E402


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    _ops.lib()
    assert torch.cuda.is_available(), "these tests need a GPU"
    return _ops


def g(seed):
    return torch.Generator().manual_seed(seed)


def gg(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def relerr(got, want):
    """max |got - want| / max |want|, in fp64 on the device of ``want``."""
    got, want = got.detach().to(want.device, torch.float64), want.detach().double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-30))


def same_bits(a, b):
    """Bitwise equality (fp32 through int32, bf16 through int16: -0 != +0 and NaN == NaN of the same payload)."""
    view = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
    return (a.shape == b.shape and a.dtype == b.dtype
            and torch.equal(a.contiguous().view(view[a.dtype]), b.contiguous().view(view[b.dtype])))


def _inputs(rows, dim, seed):
    x = torch.randn(rows, dim, device="cuda", generator=gg(seed)) * 2 + 0.5
    gam = torch.randn(dim, device="cuda", generator=gg(seed + 1)) * 0.1 + 1
    bet = torch.randn(dim, device="cuda", generator=gg(seed + 2)) * 0.1
    dy = torch.randn(rows, dim, device="cuda", generator=gg(seed + 3))
    add = torch.randn(rows, dim, device="cuda", generator=gg(seed + 4))
    return x, gam, bet, dy, add


def _reference(x, gam, bet, dy):
    """fp64 autograd on the device of x: (dx without dx_add, dgamma, dbeta)."""
    xr = x.double().requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    ln_oracle(xr, gr, br).backward(dy.double())
    return xr.grad, gr.grad, br.grad


def _split_out(ops, rows, dim, nseg):
    """A _split_buffer of nseg segments: NaN in its rows, zeros in its pad rows up to pad32(rows) (as the model's has)."""
    full = torch.empty(ops.pad32(rows), nseg * dim, dtype=torch.bfloat16, device="cuda")
    full[:rows].fill_(float("nan"))
    full[rows:].zero_()
    return full


DIMS = [64, 192, 384, 768, 1000, 1028, 2048]      # VPL 1 (idle lanes) | the model's widths | ragged VPL 4 | first VPL 8 | ABI max
ROWS = [5, 394, 12611]                            # 12 611: > 3 rows per wave at any occupancy, not a multiple of 32
SPLIT_DIMS = (192, 768, 1000)                     # the model takes the split form for D <= 1024


def _run_forms(ops, rows, dim, dydt, seed=1):
    """Forms (a)-(d) on the same inputs; (c) for both segment counts where the model uses it.  -> (inputs, results)."""
    x, gam, bet, dy, add = _inputs(rows, dim, seed)
    dyk = dy.to(dydt)
    _, mean, rstd = ops.layernorm_fwd(x, dim, rows, dim, gam, bet, torch.float32)
    res = {}

    def bwd(**kw):
        dx = torch.full((rows, dim), float("nan"), device="cuda")
        dg, db = ops.layernorm_bwd(dyk, x, dim, gam, mean, rstd, add, dx, dim, rows, dim, **kw)
        return dx, dg.clone(), db.clone()

    res["a"] = bwd()
    cs = torch.full((dim,), float("nan"), device="cuda")
    res["d"] = bwd(dx_colsum=cs) + (cs,)
    cs = torch.full((dim,), float("nan"), device="cuda")
    dx16 = torch.full((rows, dim), float("nan"), dtype=torch.bfloat16, device="cuda")
    res["b"] = bwd(dx16=dx16, dx_colsum=cs) + (cs, dx16)
    if dim in SPLIT_DIMS:
        for nseg in (3, 6):
            cs = torch.full((dim,), float("nan"), device="cuda")
            full = _split_out(ops, rows, dim, nseg)
            with ops.segments(nseg):
                res[f"c{nseg}"] = bwd(dx_split=full[:rows], dx_colsum=cs) + (cs, full)
    return (x, gam, bet, dyk, add, mean, rstd), res


# ---------------------------------------------------------------- (a)-(d): fp64 values and the identities between the forms
# every (rows, dim) with bf16 dy (the bf16 step's form); fp32 dy (the split modes' form) at every width for the small row counts
# and, in the grid-stride case, at the split widths and the ABI maximum
FORM_CASES = ([(r, d, torch.bfloat16) for r in ROWS for d in DIMS]
              + [(r, d, torch.float32) for r in ROWS for d in DIMS if r < 4096 or d in SPLIT_DIMS + (2048,)])


@pytest.mark.parametrize("rows,dim,dydt", FORM_CASES)
def test_layernorm_bwd_fused_outputs(ops, rows, dim, dydt):
    (x, gam, bet, dyk, add, mean, rstd), res = _run_forms(ops, rows, dim, dydt)
    dx_ref, dg_ref, db_ref = _reference(x, gam, bet, dyk)       # dy rounded to bf16 first when the kernel reads bf16
    dx_ref = dx_ref + add.double()
    dx, dg, db = res["a"]
    # per-row arithmetic (two wave sums over dim) and fp32 column sums over the rows: the existing bar of test_layernorm_fwd_bwd
    # holds at 12 611 rows (measured max over these cases: dx 1.3e-7, dgamma 4.2e-7, dbeta 3.6e-7)
    assert relerr(dx, dx_ref) < 5e-6
    assert relerr(dg, dg_ref) < 5e-6
    assert relerr(db, db_ref) < 5e-6
    for form, out in res.items():                              # the by-products change nothing the plain form writes
        assert same_bits(out[0], dx) and same_bits(out[1], dg) and same_bits(out[2], db), form
    colsum = res["d"][3]
    col64 = dx.double().sum(0)
    # fp32 sums of the kernel's own dx (a few rows per wave, a 4-wave tree, then the finishing reduce) vs fp64 sums of the same dx:
    # measured <= 3.4e-7;  against the fp64 reference's column sums (the dx error adds in), measured <= 3.5e-7
    assert relerr(colsum, col64) < 2e-6
    assert relerr(colsum, dx_ref.sum(0)) < 5e-6
    for form in [f for f in res if f != "d"]:
        if form != "a":
            assert same_bits(res[form][3], colsum), form
    assert same_bits(res["b"][4], dx.to(torch.bfloat16))        # dx16 is the RNE rounding ops.cast performs
    for nseg in (3, 6):
        if f"c{nseg}" not in res:
            continue
        full = res[f"c{nseg}"][4]
        with ops.segments(nseg):
            want = ops.split_ex(dx, rows, dim)
        assert same_bits(full[:rows], want), nseg               # the pieces split_ex writes, in its segment order
        assert not bool(full[rows:].any()), nseg                # the pad rows the TN product contracts over stay zero


# ---------------------------------------------------------------- (e): the classification head's strided cls rows
@pytest.mark.parametrize("B,T", [(5, 197), (394, 197), (12611, 3)])
@pytest.mark.parametrize("dim", [64, 768, 1000, 2048])
@pytest.mark.parametrize("dydt", [torch.bfloat16, torch.float32])
def test_layernorm_bwd_strided_cls_rows(ops, B, T, dim, dydt):
    x = torch.randn(B, T, dim, device="cuda", generator=gg(7)) * 2 + 0.5
    gam = torch.randn(dim, device="cuda", generator=gg(8)) * 0.1 + 1
    bet = torch.randn(dim, device="cuda", generator=gg(9)) * 0.1
    dy = torch.randn(B, dim, device="cuda", generator=gg(10)).to(dydt)
    _, mean, rstd = ops.layernorm_fwd(x, T * dim, B, dim, gam, bet, torch.float32)
    dx = torch.full_like(x, float("nan"))
    dg, db = ops.layernorm_bwd(dy, x, T * dim, gam, mean, rstd, None, dx, T * dim, B, dim, beta=bet)
    dx_ref, dg_ref, db_ref = _reference(x[:, 0], gam, bet, dy)
    assert bool(torch.isnan(dx[:, 1:]).all())                   # only the cls rows are written
    assert relerr(dx[:, 0], dx_ref) < 5e-6                      # measured: dx 2.0e-7, dgamma 3.8e-7, dbeta 3.0e-7
    assert relerr(dg, dg_ref) < 5e-6
    assert relerr(db, db_ref) < 5e-6


# ---------------------------------------------------------------- the C ABI: accumulate, rows == 0, rejections
def _abi(ops, dy, x, gam, mean, rstd, dx, dg, db, rows, dim, *, accumulate, colsum=None, ws_bytes=None, dx_add=None):
    lib = ops.lib()
    need = lib.mv_layernorm_bwd_workspace_bytes(rows, dim)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    ops.check(lib.mv_layernorm_bwd(ops._p(dy), ops._DT[dy.dtype], ops._p(x), dim, ops._p(gam), ops._p(mean), ops._p(rstd),
                                   ops._p(dx_add), ops._p(dx), dim, ops._p(dg), ops._p(db), accumulate, ops._p(ws),
                                   need if ws_bytes is None else ws_bytes, rows, dim, None, ops._p(colsum), ops._s()),
              "layernorm_bwd", rows=rows, dim=dim)


@pytest.mark.parametrize("rows,dim", [(394, 192), (12611, 768), (12611, 1000)])
@pytest.mark.parametrize("with_colsum", [False, True])
def test_layernorm_bwd_accumulate(ops, rows, dim, with_colsum):
    x, gam, bet, dy, add = _inputs(rows, dim, 11)
    dy = dy.to(torch.bfloat16)
    _, mean, rstd = ops.layernorm_fwd(x, dim, rows, dim, gam, bet, torch.float32)
    dx0, dg0, db0 = torch.empty(rows, dim, device="cuda"), torch.empty(dim, device="cuda"), torch.empty(dim, device="cuda")
    cs0 = torch.empty(dim, device="cuda") if with_colsum else None
    _abi(ops, dy, x, gam, mean, rstd, dx0, dg0, db0, rows, dim, accumulate=0, colsum=cs0, dx_add=add)
    old_g = torch.randn(dim, device="cuda", generator=gg(12))
    old_b = torch.randn(dim, device="cuda", generator=gg(13))
    dx1, dg1, db1 = torch.empty(rows, dim, device="cuda"), old_g.clone(), old_b.clone()
    cs1 = torch.full((dim,), 1e30, device="cuda") if with_colsum else None      # garbage: the column sums are overwritten
    _abi(ops, dy, x, gam, mean, rstd, dx1, dg1, db1, rows, dim, accumulate=1, colsum=cs1, dx_add=add)
    assert same_bits(dx1, dx0)
    assert same_bits(dg1, old_g + dg0) and same_bits(db1, old_b + db0)   # the same per-column sum, then one fp32 add
    if with_colsum:
        assert same_bits(cs1, cs0)


@pytest.mark.parametrize("with_colsum", [False, True])
def test_layernorm_bwd_zero_rows(ops, with_colsum):
    dim = 768
    x, gam, bet, dy, _ = _inputs(4, dim, 14)
    mean, rstd = torch.zeros(4, device="cuda"), torch.ones(4, device="cuda")
    dx = torch.full((4, dim), float("nan"), device="cuda")
    old = torch.randn(3, dim, device="cuda", generator=gg(15))
    outs = old.clone()
    _abi(ops, dy, x, gam, mean, rstd, dx, outs[0], outs[1], 0, dim, accumulate=1, colsum=outs[2] if with_colsum else None)
    assert same_bits(outs[:2], old[:2])                         # accumulate: unchanged
    if with_colsum:
        assert not bool(outs[2].any())                          # the column sums are overwritten: zero rows sum to zero
    outs = old.clone()
    _abi(ops, dy, x, gam, mean, rstd, dx, outs[0], outs[1], 0, dim, accumulate=0, colsum=outs[2] if with_colsum else None)
    assert not bool(outs[:2].any())
    assert bool(outs[2].eq(0).all()) if with_colsum else same_bits(outs[2], old[2])
    assert bool(torch.isnan(dx).all())                          # dx untouched


def test_layernorm_bwd_rejections(ops):
    rows = 8
    for dim in (66, 2052):                                      # dim % 4 != 0; dim above the ABI's 2 048
        ld = (dim + 3) // 4 * 4                                 # valid row strides: only dim itself is out of the contract
        x, dy, dx = (torch.randn(rows, ld, device="cuda") for _ in range(3))
        mean, rstd = torch.zeros(rows, device="cuda"), torch.ones(rows, device="cuda")
        with pytest.raises(RuntimeError, match="layernorm_bwd"):
            ops.layernorm_bwd(dy, x, ld, torch.ones(ld, device="cuda"), mean, rstd, None, dx, ld, rows, dim)
    dim = 768
    x, gam, bet, dy, _ = _inputs(rows, dim, 16)
    _, mean, rstd = ops.layernorm_fwd(x, dim, rows, dim, gam, bet, torch.float32)
    dx, dg, db = torch.empty(rows, dim, device="cuda"), torch.empty(dim, device="cuda"), torch.empty(dim, device="cuda")
    need = ops.lib().mv_layernorm_bwd_workspace_bytes(rows, dim)
    with pytest.raises(RuntimeError, match="layernorm_bwd"):
        _abi(ops, dy, x, gam, mean, rstd, dx, dg, db, rows, dim, accumulate=0, ws_bytes=need - 4)
    lib = ops.lib()
    split = torch.zeros(ops.pad32(rows), 6 * dim, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    for nseg in (0, 4, 2):
        with pytest.raises(RuntimeError, match="layernorm_bwd_split"):
            ops.check(lib.mv_layernorm_bwd_split(ops._p(dy), ops._DT[dy.dtype], ops._p(x), dim, ops._p(gam), ops._p(mean),
                                                 ops._p(rstd), None, ops._p(dx), dim, ops._p(dg), ops._p(db), 0, ops._p(ws), need,
                                                 rows, dim, ops._p(split), nseg, None, ops._s()), "layernorm_bwd_split")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- block hand-off: attn_block -> mlp_block
PRECS = ["bf16", "bf16x3", "bf16x3h", "fp32"]


def _side_kind(prec):
    return "bf16" if prec == "bf16" else ("split", 3 if prec in ("bf16x3", "bf16x3h") else 6)


@pytest.fixture(scope="module")
def block_params():
    D, H, Hd, B, T = 384, 6, 1536, 4, 197                       # ViT-S widths: M = 788 rows, every dim a multiple of 64
    p = {"g1": torch.randn(D, generator=g(20)) * 0.1 + 1, "b1": torch.randn(D, generator=g(21)) * 0.1,
         "wqkv": torch.randn(3 * D, D, generator=g(22)) * D ** -0.5, "bqkv": torch.randn(3 * D, generator=g(23)) * 0.1,
         "wo": torch.randn(D, D, generator=g(24)) * D ** -0.5, "bo": torch.randn(D, generator=g(25)) * 0.1,
         "g2": torch.randn(D, generator=g(26)) * 0.1 + 1, "b2": torch.randn(D, generator=g(27)) * 0.1,
         "w1": torch.randn(Hd, D, generator=g(28)) * D ** -0.5, "bf1": torch.randn(Hd, generator=g(29)) * 0.1,
         "w2": torch.randn(D, Hd, generator=g(30)) * Hd ** -0.5, "bf2": torch.randn(D, generator=g(31)) * 0.1}
    x = torch.randn(B, T, D, generator=g(32))
    r = torch.randn(B, T, D, generator=g(33))
    return {k: v.cuda() for k, v in p.items()}, x.cuda(), r.cuda(), H


def _block_pair_grads(params, x0, r, heads, p1, p2, handoff, monkeypatch):
    from myrtle_vision.hip import functional as F
    taken = []
    real_take, real_pub = F._take_side, F._publish_side

    def spy(dout, rows, dim, *kind):
        got = real_take(dout, rows, dim, *kind)
        taken.append(got[0] is not None)
        return got
    monkeypatch.setattr(F, "_take_side", spy)
    monkeypatch.setattr(F, "_publish_side", real_pub if handoff else (lambda *a, **k: None))
    ps = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    x = x0.clone().requires_grad_(True)
    D = x.shape[-1]
    F.chain_reset()
    h = F.attn_block(x, ps["g1"], ps["b1"], ps["wqkv"], ps["bqkv"], ps["wo"], ps["bo"], heads, (D // heads) ** -0.5, p1)
    arriving = []
    h.register_hook(lambda gr: arriving.append(gr.detach().clone()))
    out = F.mlp_block(h, ps["g2"], ps["b2"], ps["w1"], ps["bf1"], ps["w2"], ps["bf2"], p2)
    (out * r).sum().backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {k: v.grad for k, v in ps.items()}
    grads["x"] = x.grad
    return grads, arriving[0], taken


@pytest.mark.parametrize("p2", PRECS)
@pytest.mark.parametrize("p1", PRECS)
def test_block_handoff_matches_no_handoff(ops, block_params, p1, p2, monkeypatch):
    """attn_block (p1) -> mlp_block (p2): the mlp block's LayerNorm backward publishes dx's bf16 copy or pieces and column sums, and
    the attn block takes them when they are of its own kind.  With the hand-off disabled, the attn block computes its dY itself
    (ops.cast / ops.split_ex of the same dx: the same roundings), so every gradient is bit-identical -- except to_out's bias,
    which is the column sum either way, taken from fp32 dx (hand-off) or from the consumer's own dY."""
    params, x, r, heads = block_params
    on, arr, taken = _block_pair_grads(params, x, r, heads, p1, p2, True, monkeypatch)
    off, arr_off, taken_off = _block_pair_grads(params, x, r, heads, p1, p2, False, monkeypatch)
    assert same_bits(arr, arr_off)
    differ = {k: relerr(on[k], off[k]) for k in on if k != "bo" and not same_bits(on[k], off[k])}
    assert not differ, differ
    consumed = _side_kind(p1) == _side_kind(p2)
    # the attn block's take is the last one in backward order; a side of another kind must come back as (None, None)
    assert taken[-1] == consumed and not any(taken_off)
    want = arr.double().sum((0, 1))
    if consumed:
        assert relerr(on["bo"], want) < 2e-6                    # fp32 column sums of the arriving dx; measured <= 2.9e-7
    else:
        assert same_bits(on["bo"], off["bo"])
    # the consumer's own bias gradient: bf16 -- fp32 column sums of the bf16-rounded dY (2^-9 per element; measured <= 2.1e-3);
    # split -- split_ex's fp32 column sums of dx (measured <= 2.2e-7)
    if p1 == "bf16":
        assert relerr(off["bo"], want) < 2.0 ** -8
    else:
        assert relerr(off["bo"], want) < 2e-6


def test_vit_with_one_fp32_block_matches_no_handoff(ops, monkeypatch):
    """A bf16 ViT whose first MLP block runs at precision fp32 (precision is per module): that block's LayerNorm backward publishes
    [M, 6D] pieces, and the bf16 attention block in front of it must not take them as its [M, D] dY."""
    from myrtle_vision.hip import functional as F
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(3)
    vit = ViT(decoder="classification", image_size=224, patch_size=16, num_classes=10, dim=192, depth=2, heads=3, mlp_dim=768,
              precision="bf16", q_format="FP32").cuda()
    vit.train()
    vit.transformer.layers[0][1].fn.norm.precision = "fp32"
    img = torch.randn(2, 3, 224, 224, generator=g(40)).cuda()
    r = torch.randn(2, 10, generator=g(41)).cuda()
    real_pub = F._publish_side

    def grads(handoff):
        monkeypatch.setattr(F, "_publish_side", real_pub if handoff else (lambda *a, **k: None))
        for p in vit.parameters():
            p.grad = None
        (vit(img).float() * r).sum().backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        return {n: p.grad.detach().clone() for n, p in vit.named_parameters() if p.grad is not None}

    on, off = grads(True), grads(False)
    assert set(on) == set(off) and len(on) > 20
    # the biases the LayerNorm column sums feed (to_out / fc2 of a block that took a bf16 hand-off): fp32 sums of dx vs the
    # consumer's own sums of bf16 dY (2^-8, as above); every other gradient is bit-identical
    # (backward order: layer 1's MLP -> its attention takes bf16 dx16; its attention -> layer 0's fp32 MLP, which rejects bf16 and
    # splits dx itself; that MLP's pieces -> layer 0's bf16 attention, which rejects them and casts dx itself)
    colsum_fed = {"transformer.layers.1.0.fn.fn.to_out.0.bias"}
    assert colsum_fed <= set(on)
    differ = {n: relerr(on[n], off[n]) for n in on if n not in colsum_fed and not same_bits(on[n], off[n])}
    assert not differ, differ
    for n in colsum_fed:
        assert relerr(on[n], off[n]) < 2.0 ** -8, n            # measured 2.4e-3
