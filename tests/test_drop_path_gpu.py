"""Stochastic depth (drop path) on the device: the three kernels of csrc/drop_path.hip, the fused blocks with a per-sample scale, the
model, and the captured training step.

References: the draw is pinned bit for bit to the Philox restatement (tests/drop_path_ref.py over oracle/dropout_oracle.py); the
blocks and the model to the PARENT behaviour composed with torch ops on the device, x + c[:, None, None] * (block(x) - x), with its
gradients from autograd.  Both sides of a block comparison run the same kernels on the same operands and differ by fp32 roundings
only (the subtraction loses at most 2 ulp of max(|x|, |y|), then scaled by s = 2): forward max|out - ref| <= 1e-5 max|ref|, every
gradient relative L2 <= 1e-5 -- about 20x the derived error.  The model is held to the project's bars for its precision
(README: fp32 1e-3 logits and gradients; bf16 1.5e-2 logits, 2e-2 relative L2 per gradient tensor)."""
import numpy as np
import pytest
import torch

from drop_path_ref import Guarded, composed, draw_table

pytestmark = pytest.mark.gpu

SEED, STEP = (5 << 40) + 12345, (1 << 32) - 1            # both halves of the key in use; step + 1 carries into the counter's high word
S = float(np.float32(1.0 / 0.9))                          # a kept factor that rounds (1 / (1 - 0.1))


@pytest.fixture(scope="module")
def ops():
    from myrtle_vision.hip import ops as _ops
    return _ops


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


# ================================================================== 1. kernels
@pytest.mark.parametrize("R,B", [(3, 5), (24, 257)])
def test_draw_is_the_philox_reference_and_advances_the_step(ops, R, B):
    rates = [(0.1, 0.5, 0.9, 0.25, 0.75)[r % 5] for r in range(R)]
    thr, scale = ops.drop_path_tables(rates)
    state = torch.tensor([SEED, STEP], dtype=torch.int64).cuda()
    thr_d = torch.from_numpy(np.array(thr, dtype=np.uint32).view(np.int32)).cuda()
    scale_d = torch.tensor(scale, dtype=torch.float64).float().cuda()
    first = ops.drop_path_draw(state, thr_d, scale_d, B)
    second = ops.drop_path_draw(state, thr_d, scale_d, B)
    torch.cuda.synchronize()
    assert first.shape == (R, B) and first.data_ptr() != second.data_ptr()
    assert same_bits(first, torch.from_numpy(draw_table(rates, B, SEED, STEP)))
    assert same_bits(second, torch.from_numpy(draw_table(rates, B, SEED, STEP + 1)))
    assert state.tolist() == [SEED, STEP + 2]
    kept = float((first != 0).float().mean())
    if R * B > 1000:
        assert abs(kept - (1 - np.mean(rates))) < 0.05


def _shapes(ops, vec):
    """(3, 5, 6): samples end inside a 16-byte vector; (5, 1, 768): whole vectors; and one shape with more elements than ONE grid
    pass of the kernels' own launch: 256 threads, one vector of ``vec`` elements each, at most 8 workgroups per compute unit."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    one_pass = ops.DROP_PATH_THREADS * ops.DROP_PATH_MAX_BLOCKS_PER_CU * cus * vec
    big = (5, one_pass // (5 * 769) + 2, 769)
    assert big[0] * big[1] * big[2] > one_pass and (big[1] * big[2]) % vec != 0
    return [(3, 5, 6), (5, 1, 768), big]


def _factors(B):
    mixed = [0.0 if b % 3 == 0 else S for b in range(B)]
    return {"dropped": [0.0] * B, "kept": [S] * B, "mixed": mixed}


@pytest.mark.parametrize("which", [0, 1, 2])
def test_drop_path_add(ops, which):
    B, T, D = _shapes(ops, 4)[which]
    g = torch.Generator().manual_seed(40 + which)
    x, f = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    for name, c in _factors(B).items():
        G = Guarded(torch)
        xd, fd, cd = G.new((B, T, D), torch.float32, x), G.new((B, T, D), torch.float32, f), torch.tensor(c).cuda()
        out = ops.drop_path_add(xd, fd, cd)
        torch.cuda.synchronize()
        assert out.data_ptr() == fd.data_ptr()                                  # in place on f
        G.check()
        assert same_bits(xd, x)
        got = fd.cpu()
        cn = np.array(c, dtype=np.float32)
        want = x.double().numpy() + cn.astype(np.float64)[:, None, None] * f.double().numpy()
        for b in range(B):
            if c[b] == 0.0:
                assert same_bits(got[b], x[b]), (name, b)                       # exactly x, whatever f held
            else:
                # one fused multiply-add against the fp64 value: 1 ulp, because rounding that value to fp32 rounds a second time
                ulp = np.spacing(np.abs(want[b]).astype(np.float32)).astype(np.float64)
                assert (np.abs(got[b].double().numpy() - want[b]) <= ulp).all(), (name, b)


@pytest.mark.parametrize("din,dout", [(torch.float32, torch.float32), (torch.float32, torch.bfloat16),
                                      (torch.bfloat16, torch.bfloat16), (torch.bfloat16, torch.float32)])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_row_scale_is_bit_exact(ops, which, din, dout):
    vec = 4 if din == dout == torch.float32 else 8
    B, T, D = _shapes(ops, vec)[which]
    x = torch.randn(B, T, D, generator=torch.Generator().manual_seed(50 + which)).to(din)
    for name, c in _factors(B).items():
        G = Guarded(torch)
        xd, od, cd = G.new((B, T, D), din, x), G.new((B, T, D), dout), torch.tensor(c).cuda()
        got = ops.row_scale(xd, cd, out=od)
        torch.cuda.synchronize()
        G.check()
        want = (torch.tensor(c)[:, None, None] * x.float()).to(dout)            # evaluated on the CPU
        assert same_bits(got, want), name
        assert same_bits(xd, x)
    assert ops.row_scale(xd, cd, dout).dtype == dout and ops.row_scale(xd, cd).dtype == din


# ================================================================== 2. blocks
B_, T_, DIM, HEADS, MLP = 5, 50, 128, 2, 256


def _block_params(kind, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k)                    # noqa: E731
    if kind == "attn":
        p = dict(g=1 + r(DIM, k=0.1), b=r(DIM, k=0.1), wqkv=r(3 * DIM, DIM, k=0.08), bqkv=r(3 * DIM, k=0.1), wo=r(DIM, DIM, k=0.08),
                 bo=r(DIM, k=0.1))
    else:
        p = dict(g=1 + r(DIM, k=0.1), b=r(DIM, k=0.1), w1=r(MLP, DIM, k=0.08), b1=r(MLP, k=0.1), w2=r(DIM, MLP, k=0.08), b2=r(DIM, k=0.1))
    return {k: v.cuda() for k, v in p.items()}


def _leaves(params):
    return {k: v.clone().requires_grad_(True) for k, v in params.items()}


def _call(F, kind, x, p, prec, row_scale=None):
    kw = {} if row_scale is None else {"row_scale": row_scale}
    if kind == "attn":
        return F.attn_block(x, p["g"], p["b"], p["wqkv"], p["bqkv"], p["wo"], p["bo"], HEADS, (DIM // HEADS) ** -0.5, prec, **kw)
    return F.mlp_block(x, p["g"], p["b"], p["w1"], p["b1"], p["w2"], p["b2"], prec, **kw)


def _run(fn, params_list, x0, w):
    """fn(x, [leaf dicts]) -> out; returns (out, dx, [grad dicts]) for loss = sum(out * w)."""
    from myrtle_vision.hip import functional as F
    F.chain_reset()
    x = x0.clone().requires_grad_(True)
    leaves = [_leaves(p) for p in params_list]
    out = fn(x, leaves)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), x.grad, [{k: v.grad for k, v in lv.items()} for lv in leaves]


def _assert_close(ours, ref, tag, fwd_bar=1e-5, grad_bar=1e-5):
    out, dx, grads = ours
    rout, rdx, rgrads = ref
    err = float((out - rout).abs().max() / rout.abs().max())
    print(f"{tag}: forward {err:.2e}")
    assert err <= fwd_bar, (tag, err)
    e = rel_l2(dx, rdx)
    print(f"{tag}: dx {e:.2e}")
    assert e <= grad_bar, (tag, "dx", e)
    for g, rg in zip(grads, rgrads):
        for k in rg:
            assert g[k] is not None and rg[k] is not None, (tag, k)
            e = rel_l2(g[k], rg[k])
            print(f"{tag}: d{k} {e:.2e}")
            assert e <= grad_bar, (tag, k, e)


class _Spy:
    """Counts calls of ``ops`` functions (and keeps their keyword arguments) while the block functions run."""

    def __init__(self, monkeypatch, ops, names):
        self.calls = {n: [] for n in names}
        for n in names:
            monkeypatch.setattr(ops, n, self._wrap(n, getattr(ops, n)))

    def _wrap(self, name, fn):
        def run(*a, **kw):
            r = fn(*a, **kw)
            self.calls[name].append((a, kw, r))
            return r
        return run


# (precision, f32 gemm mode, internal path)
PATHS = [("bf16", "bf16x6", "bf16"), ("fp32", "bf16x6", "split"), ("bf16x3", "bf16x6", "split"), ("fp32", "mfma", "plain")]


@pytest.mark.parametrize("prec,mode,path", PATHS, ids=[f"{p}-{m}" for p, m, _ in PATHS])
@pytest.mark.parametrize("kind", ["attn", "mlp"])
def test_block_with_row_scale_equals_the_composed_parent(ops, monkeypatch, kind, prec, mode, path):
    from myrtle_vision.hip import functional as F
    assert ops.x6_block_ok(B_ * T_, DIM, 3 * DIM, MLP)                          # the split-operand path exists at this size
    g = torch.Generator().manual_seed(7)
    x0, w = torch.randn(B_, T_, DIM, generator=g).cuda(), torch.randn(B_, T_, DIM, generator=g).cuda()
    c = torch.tensor([0.0, 2.0, 2.0, 0.0, 2.0]).cuda()
    params = _block_params(kind, 11)
    prev = ops.set_f32_gemm(mode)
    try:
        ref = _run(lambda x, lv: composed(lambda t: _call(F, kind, t, lv[0], prec), x, c), [params], x0, w)
        spy = _Spy(monkeypatch, ops, ["nt_x6", "linear_fwd", "drop_path_add", "row_scale", "split_ex", "cast"])
        ours = _run(lambda x, lv: _call(F, kind, x, lv[0], prec, c), [params], x0, w)
    finally:
        ops.set_f32_gemm(prev)
    # which internal path ran
    assert len(spy.calls["drop_path_add"]) == 1 and len(spy.calls["row_scale"]) == 1
    scaled = spy.calls["row_scale"][0][2]
    if path == "bf16":
        assert scaled.dtype == torch.bfloat16 and not spy.calls["nt_x6"] and not spy.calls["split_ex"]
        assert spy.calls["linear_fwd"][-1][1].get("epi", ops.EPI_NONE) == ops.EPI_NONE
    elif path == "split":
        assert scaled.dtype == torch.float32 and not spy.calls["linear_fwd"]
        fwd = [kw for a, kw, _ in spy.calls["nt_x6"] if a[2] == "fwd"]
        assert fwd[-1]["residual"] is None
        # the split of the scaled gradient, with the output bias' column sums
        assert any(a[0].data_ptr() == scaled.data_ptr() and kw.get("colsum_out") is not None for a, kw, _ in spy.calls["split_ex"])
    else:
        assert scaled.dtype == torch.float32 and not spy.calls["nt_x6"] and not spy.calls["split_ex"]
        assert spy.calls["linear_fwd"][-1][1].get("epi", ops.EPI_NONE) == ops.EPI_NONE
    # dropped samples leave the block as they entered it
    assert same_bits(ours[0][0], x0[0]) and same_bits(ours[0][3], x0[3])
    _assert_close(ours, ref, f"{kind}/{prec}/{path}")


def test_row_scale_none_is_the_parent_block(ops, monkeypatch):
    """row_scale=None: none of the new ops runs, and the block's bits are those of the call without the keyword."""
    from myrtle_vision.hip import functional as F
    g = torch.Generator().manual_seed(8)
    x0, w = torch.randn(B_, T_, DIM, generator=g).cuda(), torch.randn(B_, T_, DIM, generator=g).cuda()
    for kind in ("attn", "mlp"):
        params = _block_params(kind, 12)
        a = _run(lambda x, lv: _call(F, kind, x, lv[0], "bf16"), [params], x0, w)
        spy = _Spy(monkeypatch, ops, ["drop_path_add", "row_scale", "drop_path_draw"])
        b = _run(lambda x, lv: (F.attn_block(x, *[lv[0][k] for k in ("g", "b", "wqkv", "bqkv", "wo", "bo")], HEADS,
                                             (DIM // HEADS) ** -0.5, "bf16", row_scale=None) if kind == "attn" else
                                F.mlp_block(x, *[lv[0][k] for k in ("g", "b", "w1", "b1", "w2", "b2")], "bf16", row_scale=None)),
                 [params], x0, w)
        assert not any(spy.calls.values())
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and all(same_bits(a[2][0][k], b[2][0][k]) for k in a[2][0])


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
@pytest.mark.parametrize("factors", [[1.0] * 5, [0.0, 2.0, 2.0, 0.0, 2.0]], ids=["kept-1.0", "mixed-2.0"])
def test_output_bias_gradient_when_a_plain_block_follows(ops, prec, factors):
    """The forward link between blocks: the plain block's LayerNorm backward writes the column sums of ITS dx into the bias its
    producer named -- right for a plain producer, wrong for a drop-path one (colsum(c * dout)), which therefore names none.
    (With the link left on, the mixed case's dbo is off by O(1).)  fp32: the blocks' bars.  bf16: the second block rounds ITS input's
    LayerNorm to bf16, so an fp32-ulp difference between the two sides flips a rounding here and there (2^-9 of an element each);
    two blocks in a row are a model, held to the project's bf16 bars (README: 1.5e-2 of max |out|, 2e-2 relative L2 per gradient)."""
    from myrtle_vision.hip import functional as F
    g = torch.Generator().manual_seed(9)
    x0, w = torch.randn(B_, T_, DIM, generator=g).cuda(), torch.randn(B_, T_, DIM, generator=g).cuda()
    c = torch.tensor(factors).cuda()
    pa, pm = _block_params("attn", 13), _block_params("mlp", 14)
    ref = _run(lambda x, lv: _call(F, "mlp", composed(lambda t: _call(F, "attn", t, lv[0], prec), x, c), lv[1], prec), [pa, pm], x0, w)
    ours = _run(lambda x, lv: _call(F, "mlp", _call(F, "attn", x, lv[0], prec, c), lv[1], prec), [pa, pm], x0, w)
    e = rel_l2(ours[2][0]["bo"], ref[2][0]["bo"])
    print(f"chain/{prec}: dbo {e:.2e}")
    _assert_close(ours, ref, f"chain/{prec}", *((1e-5, 1e-5) if prec == "fp32" else BARS["bf16"]))


def _micro(**kw):
    from myrtle_vision.models.vit import ViT
    base = dict(decoder="classification", image_size=224, patch_size=16, num_classes=10, dim=128, depth=3, heads=2, mlp_dim=256)
    base.update(kw)
    return ViT(**base)


def test_drop_path_function_on_the_module_path(ops, monkeypatch):
    """A fake-quantised format runs the Residual module by module: F.drop_path scales the branch, same reference, same bars."""
    from myrtle_vision.hip import functional as F
    torch.manual_seed(3)
    vit = _micro(q_format="FP16_32", precision="fp32").cuda().train()
    res = vit.transformer.layers[1][1]
    g = torch.Generator().manual_seed(10)
    x0, w = torch.randn(B_, T_, DIM, generator=g).cuda(), torch.randn(B_, T_, DIM, generator=g).cuda()
    c = torch.tensor([0.0, 2.0, 2.0, 0.0, 2.0]).cuda()
    names = [n for n, _ in res.named_parameters()]

    def run(fn):
        F.chain_reset()
        vit.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        with ops.segments(ops.prec_segments("fp32")):
            out = fn(x)
        (out * w).sum().backward()
        torch.cuda.synchronize()
        return out.detach(), x.grad, [{n: p.grad.clone() for n, p in res.named_parameters()}]

    ref = run(lambda x: composed(res, x, c))
    spy = _Spy(monkeypatch, ops, ["row_scale", "drop_path_add"])
    fused = _Spy(monkeypatch, F, ["mlp_block", "attn_block"])
    ours = run(lambda x: res(x, c))
    assert len(spy.calls["row_scale"]) == 2 and not spy.calls["drop_path_add"] and not any(fused.calls.values())   # forward + backward
    assert names and set(ours[2][0]) == set(names)
    _assert_close(ours, ref, "module path")
    y = torch.randn(B_, 7, generator=g).cuda().to(torch.bfloat16)
    assert F.drop_path(y, c).dtype == torch.bfloat16 and F.drop_path(y, None) is y


# ================================================================== 3. model
BARS = {"fp32": (1e-3, 1e-3), "bf16": (1.5e-2, 2e-2)}                         # README: logits (of max |logit|), relative L2 per gradient
MODEL_SEED = 977


def _pair(prec, rate=0.5, **kw):
    """(model with drop path, plain model) with the same weights."""
    torch.manual_seed(31)
    plain = _micro(precision=prec, q_format="FP32").cuda()
    dp = _micro(precision=prec, q_format="FP32", drop_path_rate=rate, **kw).cuda()
    dp.load_state_dict(plain.state_dict())
    return dp, plain


def _batch(B=6, seed=17):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 3, 224, 224, generator=g).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()


def _manual(plain, img, table, rows):
    """The plain model's forward with every branch that has a row composed by hand: x + c * (branch(x) - x)."""
    tr = plain.transformer

    def forward(x):
        for i, blk in enumerate(tr.layers):
            for j in (0, 1):
                x = composed(blk[j], x, table[rows[(i, j)]]) if (i, j) in rows else blk[j](x)
        return x
    tr.forward = forward
    try:
        return plain(img)
    finally:
        del tr.forward


def _loss_grads(model, logits, labels):
    from myrtle_vision.hip.functional import cross_entropy
    model.zero_grad(set_to_none=True)
    loss = cross_entropy(logits, labels)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_model_training_forward_and_gradients(ops, prec):
    dp, plain = _pair(prec)
    dp.train(), plain.train()
    img, labels = _batch()
    tr = dp.transformer
    assert tr.block_drop_rates == [0.0, 0.25, 0.5] and tr.last_table is None
    tr.drop_path.seed(MODEL_SEED)
    logits = dp(img)
    assert tr.drop_path.state.tolist() == [MODEL_SEED, 1]
    table = tr.last_table
    assert same_bits(table, torch.from_numpy(draw_table([0.25, 0.25, 0.5, 0.5], 6, MODEL_SEED, 0)))
    assert 0 < int((table == 0).sum()) < table.numel()                          # the seed drops some and keeps some
    _, grads = _loss_grads(dp, logits, labels)
    ref_logits = _manual(plain, img, table, tr.drop_path_rows)
    _, ref_grads = _loss_grads(plain, ref_logits, labels)
    tol_logits, tol_grad = BARS[prec]
    err = float((logits.detach() - ref_logits.detach()).abs().max() / ref_logits.detach().abs().max())
    print(f"model/{prec}: logits {err:.2e}")
    assert err < tol_logits
    assert set(grads) == set(ref_grads)
    for n in ref_grads:
        e = rel_l2(grads[n], ref_grads[n])
        print(f"model/{prec}: {n} {e:.2e}")
        assert e < tol_grad, (n, e)
    # a second forward draws the next table into new memory: the first one is still what its backward would read
    dp(img)
    assert tr.last_table.data_ptr() != table.data_ptr()
    assert same_bits(tr.last_table, torch.from_numpy(draw_table([0.25, 0.25, 0.5, 0.5], 6, MODEL_SEED, 1)))


def test_model_eval_and_rate_zero_are_the_parent_bits(ops, monkeypatch):
    dp, plain = _pair("bf16")
    img, labels = _batch()
    dp.eval(), plain.eval()
    with torch.no_grad():
        assert same_bits(dp(img), plain(img))
    assert dp.transformer.last_table is None and dp.transformer.drop_path.state is None
    zero, plain = _pair("bf16", rate=0.0)
    zero.train(), plain.train()

    def boom(*a, **kw):
        raise AssertionError("a drop-path op ran with the rate at 0")
    for name in ("drop_path_draw", "drop_path_add", "row_scale"):
        monkeypatch.setattr(ops, name, boom)
    la, ga = _loss_grads(zero, zero(img), labels)
    lb, gb = _loss_grads(plain, plain(img), labels)
    assert same_bits(la, lb) and set(ga) == set(gb) and all(same_bits(ga[n], gb[n]) for n in ga)


def test_model_with_pruned_tail(ops, monkeypatch):
    from myrtle_vision.hip import functional as F
    pruned, _ = _pair("bf16", prune_dead_tokens=True)
    full, _ = _pair("bf16")
    pruned.train(), full.train()
    img, _ = _batch()
    for m in (pruned, full):
        m.transformer.drop_path.seed(MODEL_SEED)
    spy = _Spy(monkeypatch, F, ["mlp_block"])
    a = pruned(img)
    shapes = [tuple(r.shape) for _, _, r in spy.calls["mlp_block"]]
    b = full(img)
    assert shapes == [(6, 197, 128), (6, 197, 128), (6, 1, 128)]                 # the last FeedForward ran on the cls rows
    assert spy.calls["mlp_block"][2][1]["row_scale"].shape == (6,)               # with its samples' factors
    assert same_bits(pruned.transformer.last_table, full.transformer.last_table)
    err = float((a - b).abs().max() / b.abs().max())
    print(f"pruned tail: logits {err:.2e}")
    assert err < BARS["bf16"][0]


def test_converted_int8_residual_refuses_a_scale(ops):
    torch.manual_seed(1)
    vit = _micro(precision="bf16", q_format="FP32").cuda()
    vit.quantizer.prepare_qat("PyTorchINT8")
    img, _ = _batch(4)
    with torch.no_grad():
        vit(img)
    vit.convert()
    vit.eval()
    x = torch.randn(4, 197, 128).cuda()
    c = torch.ones(4).cuda()
    for j in (0, 1):
        res = vit.transformer.layers[0][j]
        with torch.no_grad():
            assert res(x).shape == x.shape
            with pytest.raises(ValueError):
                res(x, c)


# ================================================================== 4. captured step
def test_captured_step_draws_a_new_table_on_every_replay(ops):
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import AdamW, ParamArena
    from myrtle_vision.utils.utils import seed_everything
    rates = [0.25, 0.25, 0.5, 0.5]
    batches = [_batch(6, 60 + i) for i in range(4)]
    loss_fn = lambda m, x, y: cross_entropy(m(x), y)                            # noqa: E731

    def build():
        seed_everything(23)
        vit = _micro(precision="bf16", q_format="FP32", drop_path_rate=0.5).cuda().train()
        vit.transformer.drop_path.seed(MODEL_SEED)
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05)
        return vit, opt

    vit_e, opt_e = build()
    losses_e = []
    for i in [0, 0, 0, 1, 2, 3]:
        opt_e.zero_grad()
        loss = loss_fn(vit_e, *batches[i])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
    vit_g, opt_g = build()
    graphed = GraphedTrainStep(vit_g, opt_g, loss_fn, *batches[0], warmup=3)
    tr = vit_g.transformer
    assert tr.drop_path.state.tolist() == [MODEL_SEED, 3]                       # three warm-up steps; the capture itself ran nothing
    losses_g, tables = [], []
    for k, i in enumerate((1, 2, 3)):
        losses_g.append(float(graphed(*batches[i])))
        torch.cuda.synchronize()
        assert tr.drop_path.state.tolist() == [MODEL_SEED, 4 + k]
        tables.append(tr.last_table.clone())
        assert same_bits(tables[-1], torch.from_numpy(draw_table(rates, 6, MODEL_SEED, 3 + k)))
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])
    assert losses_g == losses_e[3:]
    assert torch.equal(opt_g.arena.flat_param, opt_e.arena.flat_param)
