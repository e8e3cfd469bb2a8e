"""What the per-family attention test files (tests/test_attention_long.py: 64-wide bf16, _long_f16.py: half operands of "bf16x3h",
_long_f32.py: exact fp32, test_attention_dh.py: bf16 at widths 32 and 128), tests/test_attention_tiled.py and
tests/test_launch_order_gpu.py share: the family table, every numeric bar (once, under a name), the input builder, the fp64
reference, the error measures, the check against fp64, the bodies of the tests every family repeats, and the model / graph-capture
helpers.  Not a test file: the four files keep their test names and cases and call in here.

A new attention family (another operand precision, another head width) is one more entry of ``FAMILIES`` -- its width, operand,
wrappers, caps and bars -- and a test file that lists its shapes."""
from contextlib import contextmanager
from dataclasses import dataclass

import pytest
import torch

from oracle.detinit import det_images, det_labels, det_param
from oracle.vit_oracle import ViTConfig, loss_and_grads
from test_attention_short import g, ops, rel_l2, same_bits  # noqa: F401  (re-exported: one copy of each)
from test_vit_parity import report

# ================================================================== the bars
# Whole-tensor relative L2 errors against fp64 on the same rounded inputs (tests/test_hip_ops.py's attention bars): out, lse
# (largest absolute), grad (each of dq / dk / dv), colsum_own (the column sums against the sums of the returned dqkv), colsum64
# (against fp64).  perm_*: a key permutation against the unpermuted run.  spike: one query with scores ~30x the rest.
# model_*: a whole model against the CPU oracle (logits by max |logit|, every gradient tensor by relative L2); mat_*: the same
# model on the key-tiled kernels against the materialised path.
_BF16 = dict(out=1.5e-2, lse=1e-4, grad=3e-2, colsum_own=5e-3, colsum64=3e-2,
             perm_out=6e-3, perm_lse=1e-4, perm_grad=2e-2,
             model_logits=1.5e-2, model_grad=2e-2, mat_logits=6e-3, mat_grad=2e-2)
_HALF = dict(out=6e-4, lse=2e-5, grad=2e-3, colsum_own=1e-5,
             perm_out=6e-4, perm_lse=2e-5, perm_grad=3e-3,
             model_logits=1e-3, model_grad=1e-3)
OUT_BAR, LSE_BAR, GRAD_BAR, SPIKE_BAR = 2e-6, 2e-5, 5e-6, 5e-5      # test_hip_ops.py's fp32 attention bars
_FP32 = dict(out=OUT_BAR, lse=LSE_BAR, grad=GRAD_BAR,
             perm_out=OUT_BAR, perm_lse=LSE_BAR, perm_grad=GRAD_BAR, spike=SPIKE_BAR,
             model_logits=1e-3, model_grad=1e-3, mat_logits=1e-5, mat_grad=1e-4)
BARS = {"bf16": _BF16, "half": _HALF, "fp32": _FP32}                 # by arithmetic: the widths 32 and 128 are bf16's
HALF_VS_FP32 = 1e-3              # bf16x3h against the fp32 mode: logits and every gradient tensor
INT8_MICRO_BAR = 1.5e-2          # the converted int8 model against the int8 oracle (tests/test_int8_model.py's micro bar)
# ViT-B/16 at 384^2, batch 64: a slice of the batch against the whole (bf16: relative L2; bf16x3h: relative L2 and max-norm), the
# loss and the gradient of the batch against the mean of its halves
VITB = dict(bf16_sample=1e-5, half_sample=2e-3, loss_halves=1e-5, grad_halves=2e-4)


# ================================================================== the families
@dataclass(frozen=True)
class Family:
    name: str
    dh: int                      # head width
    arith: str                   # "bf16" | "half" | "fp32": the operand rounding, the builder of make() and the key of BARS
    amp: float                   # standard deviation of q / k / v
    fwd: tuple                   # ops' dispatching forward wrapper(s): with lse [, without]
    bwd: str                     # ... and backward wrapper
    long_fwd: str                # the key-tiled kernels called directly (None: the dispatching wrappers are the only ones)
    long_bwd: str
    whole_head: str              # the whole-head C entry point of the forward, and the longest N it takes
    cap: int
    qk_mult: float               # q and k this much larger: the running maximum of a row really moves between key blocks
    precision: str               # the model precision whose blocks run this family
    n2_fraction: int             # "no N^2 tensor": peak growth stays under 1 / this of one [B, H, N, N] fp32 tensor

    @property
    def bars(self):
        return BARS[self.arith]

    @property
    def scale(self):
        return self.dh ** -0.5

    def _bind(self, ops, name):
        """ops.<name> as f(..., B, N, H, scale, **kw), looked up at call time (tests monkeypatch ops)"""
        if name.endswith("_dh"):
            return lambda *a, **kw: getattr(ops, name)(*a[:-1], self.dh, a[-1], **kw)
        return lambda *a, **kw: getattr(ops, name)(*a, **kw)

    def forward(self, ops, long=False):
        return self._bind(ops, self.long_fwd if long else self.fwd[0])

    def forward_plain(self, ops, long=False):
        """fp32 only: the evaluation form, without the lse"""
        if long:
            return lambda *a: getattr(ops, self.long_fwd)(*a, lse=False)
        return self._bind(ops, self.fwd[1])

    def backward(self, ops, long=False):
        return self._bind(ops, self.long_bwd if long else self.bwd)


FAMILIES = {f.name: f for f in (
    Family("bf16", 64, "bf16", 1.5, ("attention_fwd",), "attention_bwd", "attention_fwd_long", "attention_bwd_long",
           "mv_attention_fwd", 320, 4.0, "bf16", 4),
    Family("half", 64, "half", 1.2, ("attention_fwd_f16",), "attention_bwd_f16", "attention_fwd_long_f16", "attention_bwd_long_f16",
           "mv_attention_fwd_f16", 288, 3.0, "bf16x3h", 4),
    Family("fp32", 64, "fp32", 1.5, ("attention_fwd_f32_lse", "attention_fwd_f32"), "attention_bwd_f32_fused",
           "attention_fwd_long_f32", "attention_bwd_long_f32", "mv_attention_fwd_f32_lse", 272, 2.0, "fp32", 2),
    Family("dh32", 32, "bf16", 1.5, ("attention_fwd_dh",), "attention_bwd_dh", None, None, None, None, 4.0, "bf16", 4),
    Family("dh128", 128, "bf16", 1.5, ("attention_fwd_dh",), "attention_bwd_dh", None, None, None, None, 4.0, "bf16", 4),
)}


# ================================================================== inputs, reference, error measures
def relerr(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def attn_ref(qkv, H, dh):
    B, N, _ = qkv.shape
    q, k, v = qkv.double().view(B, N, 3, H, dh).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-2, -1)) * dh ** -0.5
    return (s.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * dh), torch.logsumexp(s, dim=-1)


def make(fam, ops, B, N, H, gscale=1.0, qk_mult=1.0, seed=1):
    """-> (qkv [B, N, 3*H*dh], dout [B, N, H*dh]); qk_mult scales q and k (scores by qk_mult^2), gscale the gradient.
    bf16: both rounded to bf16, on the host.  half: q/k/v cast to half on the device, fp32 dout on the host.  fp32: both fp32,
    on the host."""
    dh = fam.dh
    qkv = torch.randn(B, N, 3, H, dh, generator=g(seed)) * fam.amp
    qkv[:, :, :2] *= qk_mult
    qkv = qkv.view(B, N, 3 * H * dh)
    dout = torch.randn(B, N, H * dh, generator=g(seed + 1)) * gscale
    if fam.arith == "bf16":
        return qkv.to(torch.bfloat16), dout.to(torch.bfloat16)
    if fam.arith == "half":
        return ops.cast_f16(qkv.cuda()), dout
    return qkv, dout


def grad_errs(got, ref, B, N, H, dh):
    """Per-part (q, k, v) relative L2 errors.  A part that is exactly zero in exact arithmetic (dq, dk at N = 1, where softmax is
    exactly 1) is held against the size of the whole gradient instead of its own."""
    got, ref = got.detach().double().cpu().view(B, N, 3, H, dh), ref.detach().double().cpu().view(B, N, 3, H, dh)
    errs = []
    for i in range(3):
        den = float(ref[:, :, i].norm())
        if den <= 1e-3 * float(ref.norm()):
            den = float(ref.norm())
        errs.append(float((got[:, :, i] - ref[:, :, i]).norm()) / den)
    return errs


def permute_keys(qkv, perm, H, dh):
    """keys and values of every head reordered by perm, queries in place"""
    B, N, _ = qkv.shape
    q5 = qkv.view(B, N, 3, H, dh)
    q5p = q5.clone()
    q5p[:, :, 1] = q5[:, perm, 1]
    q5p[:, :, 2] = q5[:, perm, 2]
    return q5p.view(B, N, 3 * H * dh).contiguous()


def materialised(fam, ops, qkv_d, dout_d, B, N, H):
    probs = ops.attention_probs_fp32(qkv_d, B, N, H, fam.dh, fam.scale)
    out = ops.attention_pv_fp32(probs, qkv_d, B, N, H, fam.dh)
    dqkv = ops.attention_bwd_fp32(probs, qkv_d, dout_d, B, N, H, fam.dh, fam.scale)
    return out, dqkv


# ================================================================== against fp64
def check_against_fp64(fam, ops, qkv, dout, B, N, H, long=False):
    """The family's forward and backward (long: the key-tiled kernels called directly) against fp64 autograd on the same rounded
    inputs, at the family's bars, with what each family promises beyond them."""
    ref_in = qkv.cpu().double().requires_grad_(True)
    want, lse_ref = attn_ref(ref_in, H, fam.dh)
    want.backward(dout.double())
    body = {"bf16": _check_bf16, "half": _check_half, "fp32": _check_fp32}[fam.arith]
    return body(fam, ops, qkv, dout, B, N, H, long, want, lse_ref.detach(), ref_in.grad)


def _check_bf16(fam, ops, qkv, dout, B, N, H, long, want, lse_ref, ref_grad):
    dh, scale, bars = fam.dh, fam.scale, fam.bars
    fwd, bwd = fam.forward(ops, long), fam.backward(ops, long)
    out, lse = fwd(qkv.cuda(), B, N, H, scale)
    part = torch.full((B, 3 * H * dh), float("nan"), device="cuda")
    dqkv = bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale, colsum=part)
    got, ref = dqkv.float().cpu().view(B, N, 3, H, dh), ref_grad.view(B, N, 3, H, dh)
    e_out = relerr(out.float(), want)
    e_lse = float((lse.cpu().double() - lse_ref).abs().max())
    e_g = [relerr(got[:, :, i], ref[:, :, i]) for i in range(3)]
    e_cs = relerr(part.cpu(), dqkv.float().sum(1).cpu())
    e_cs64 = relerr(part.cpu().double(), ref_grad.sum(1))
    print(f"dh={dh} B={B} N={N} H={H}: out {e_out:.3e} lse {e_lse:.3e} dq {e_g[0]:.3e} dk {e_g[1]:.3e} dv {e_g[2]:.3e} "
          f"colsum {e_cs:.3e} colsum_vs_fp64 {e_cs64:.3e}")
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(dqkv.float()).all())
    # P is rounded to bf16 before P.V (2^-9 per element, averaged over keys) and the output once more
    assert e_out < bars["out"]
    assert e_lse < bars["lse"]
    for i, (e, name) in enumerate(zip(e_g, "qkv")):
        if float(ref[:, :, i].abs().max()) == 0.0:
            # N = 1: p = 1, so dS = p (dP - delta) and with it dq and dk are exactly 0 and a relative error does not exist.  dP and
            # delta are two fp32 sums of the same dh products dO_d v_d in different orders: each is within dh 2^-24 sum |dO_d v_d|
            # of the exact value, so |dS| <= 2 dh 2^-24 sum |dO_d v_d| scale, and |dq|, |dk| <= |dS| max(|k|, |q|) (one bf16
            # rounding of dS and one of the result: a factor (1 + 2^-8)^2)
            x = qkv.float().view(B, N, 3, H, dh)
            terms = (dout.float().view(B, N, H, dh).abs() * x[:, :, 2].abs()).sum(-1).max()
            bound = float(2 * dh * 2.0 ** -24 * terms * scale * x[:, :, :2].abs().max() * (1 + 2.0 ** -8) ** 2)
            print(f"  d{name}: exact value 0, largest |got| {float(got[:, :, i].abs().max()):.3e}, bound {bound:.3e}")
            assert float(got[:, :, i].abs().max()) <= bound, name
        else:
            assert e < bars["grad"], name
    assert e_cs < bars["colsum_own"]
    assert e_cs64 < bars["colsum64"]
    dq2 = bwd(qkv.cuda(), out, dout.cuda(), lse, B, N, H, scale)          # colsum is optional
    assert torch.equal(dq2, dqkv)
    return out, lse, dqkv, part


def _check_half(fam, ops, q16, dout, B, N, H, long, want, lse_ref, ref_grad):
    scale, bars = fam.scale, fam.bars
    fwd, bwd = fam.forward(ops, long), fam.backward(ops, long)
    out, lse = fwd(q16, B, N, H, scale)
    e_out = relerr(out, want)
    assert out.dtype == torch.float32 and e_out < bars["out"], e_out
    assert float((lse.cpu().double() - lse_ref).abs().max()) < bars["lse"]
    dqkv = bwd(q16, out, dout.cuda(), lse, B, N, H, scale)
    assert dqkv.dtype == torch.float32 and bool(torch.isfinite(dqkv).all())
    got, ref = dqkv.cpu().double().view(B, N, 3, H, fam.dh), ref_grad.view(B, N, 3, H, fam.dh)
    for i, name in enumerate("qkv"):
        # (N = 1: softmax is exactly 1, so dq = dk = 0 exactly; the kernels leave rounding residue of P - 1 and dP - delta, held
        # here against the size of the whole gradient)
        e = float((got[:, :, i] - ref[:, :, i]).norm() / max(float(ref[:, :, i].norm()), 1e-3 * float(ref.norm())))
        assert e < bars["grad"], (name, e)
    # the split-output form (what the bf16x3h block runs): the bf16 pieces of exactly those fp32 values, and per-image column sums
    for nseg in (3, 6):
        with ops.segments(nseg):
            part = torch.full((B, 3 * H * fam.dh), float("nan"), device="cuda")
            pieces = bwd(q16, out, dout.cuda(), lse, B, N, H, scale, split=True, colsum=part)
            assert torch.equal(pieces, ops.split_ex(dqkv.view(B * N, 3 * H * fam.dh), B * N, 3 * H * fam.dh))
        assert relerr(part, dqkv.double().sum(1)) < bars["colsum_own"]
    part = torch.full((B, 3 * H * fam.dh), float("nan"), device="cuda")
    assert torch.equal(bwd(q16, out, dout.cuda(), lse, B, N, H, scale, colsum=part), dqkv)   # colsum is optional; deterministic
    assert relerr(part, dqkv.double().sum(1)) < bars["colsum_own"]
    # an all-zero gradient gives exact zeros (scale 1, no 0 * inf)
    assert not bwd(q16, out, torch.zeros_like(dout).cuda(), lse, B, N, H, scale).any()
    return out, lse, dqkv


def _check_fp32(fam, ops, qkv, dout, B, N, H, long, want, lse_ref, ref_grad):
    """Through the dispatch (not long) also against the materialised fp32 path."""
    scale = fam.scale
    fwd_lse, fwd_plain, bwd = fam.forward(ops, long), fam.forward_plain(ops, long), fam.backward(ops, long)
    qkv_d, dout_d = qkv.cuda(), dout.cuda()
    bars = dict(out=fam.bars["out"], lse=fam.bars["lse"], grad=fam.bars["grad"])
    mat = None if long else materialised(fam, ops, qkv_d, dout_d, B, N, H)
    if N == 4097:
        # at this length only: the larger of the bar and twice the materialised fp32 path's own error against fp64 (same input);
        # the lse bar stays (the materialised path has no lse)
        bars["out"] = max(bars["out"], 2 * relerr(mat[0], want))
        bars["grad"] = max(bars["grad"], 2 * max(grad_errs(mat[1], ref_grad, B, N, H, fam.dh)))
    out, lse = fwd_lse(qkv_d, B, N, H, scale)
    assert out.dtype == torch.float32 and out.shape == (B, N, H * fam.dh) and lse.shape == (B, H, N)
    e_out = relerr(out, want)
    e_lse = float((lse.cpu().double() - lse_ref).abs().max())
    assert e_out < bars["out"], (e_out, bars)
    assert e_lse < bars["lse"], e_lse
    plain = fwd_plain(qkv_d, B, N, H, scale)
    assert torch.equal(plain, out)                                    # the evaluation form: the same bits without the lse
    assert torch.equal(fwd_lse(qkv_d, B, N, H, scale)[0], out)        # deterministic
    dqkv = bwd(qkv_d, out, dout_d, lse, B, N, H, scale)
    assert dqkv.dtype == torch.float32 and dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv).all())
    errs = grad_errs(dqkv, ref_grad, B, N, H, fam.dh)
    assert max(errs) < bars["grad"], (errs, bars)
    assert torch.equal(bwd(qkv_d, out, dout_d, lse, B, N, H, scale), dqkv)     # deterministic
    if mat is not None:                                               # the materialised fp32 path at the same bars
        assert relerr(out, mat[0]) < bars["out"]
        assert max(grad_errs(dqkv, mat[1], B, N, H, fam.dh)) < bars["grad"]
    report(f"attn_long_f32 N={N} out / lse / dq dk dv vs fp64", max([e_out] + errs))
    return out, lse, dqkv


# ================================================================== whole models
MICRO = dict(dim=192, depth=2, heads=3, mlp_dim=768)


def model_case(decoder, image_size, num_classes, batch, name, widths=MICRO):
    """-> (oracle config, ViT keyword arguments, deterministic parameters, images, labels)"""
    kw = dict(decoder=decoder, image_size=image_size, num_classes=num_classes, **widths)
    cfg = ViTConfig(patch_size=16, **kw)
    params = {k: det_param(k, s) for k, s in cfg.param_shapes().items()}
    img = det_images(name, batch, image_size)
    shape = (batch,) if decoder == "classification" else (batch, image_size, image_size)
    labels = det_labels(name, shape, num_classes)
    return cfg, kw, params, img, labels


def build_model(kw, precision, params):
    from myrtle_vision.models.vit import ViT
    vit = ViT(patch_size=16, q_format="FP32", precision=precision, **kw)
    vit.load_state_dict(params)
    return vit.cuda()


def run_model(vit, img, labels):
    """One forward + backward -> (logits, {name: gradient}) on the host, fp32"""
    from myrtle_vision.hip.functional import cross_entropy
    logits = vit(img.cuda())
    cross_entropy(logits, labels.cuda()).backward()
    torch.cuda.synchronize()
    return logits.detach().float().cpu(), {k: p.grad.float().cpu() for k, p in vit.named_parameters() if p.grad is not None}


@contextmanager
def watching(ops, count=(), forbid_probs=False, attn_long=None):
    """-> {wrapper: calls} of the ops wrappers named in count, while the block runs.  forbid_probs: the materialised attention
    must not run (ops.attention_probs_fp32 raises).  attn_long: ops.ATTN_LONG for the block."""
    calls = {name: 0 for name in count}

    def counting(name, real):
        def run(*a, **k):
            calls[name] += 1
            return real(*a, **k)
        return run

    def no_probs(*a, **k):
        raise AssertionError("materialised attention ran")

    mp = pytest.MonkeyPatch()
    try:
        if attn_long is not None:
            mp.setattr(ops, "ATTN_LONG", attn_long)
        for name in count:
            mp.setattr(ops, name, counting(name, getattr(ops, name)))
        if forbid_probs:
            mp.setattr(ops, "attention_probs_fp32", no_probs)
        yield calls
    finally:
        mp.undo()


def model_errors(logits, grads, ref_logits, ref_grads):
    """-> (logit error by max |logit|, {name: relative L2 error} of every gradient tensor the reference has)"""
    err = float((logits - ref_logits).abs().max() / ref_logits.abs().max())
    return err, {k: relerr(gr, ref_grads[k]) for k, gr in grads.items() if ref_grads.get(k) is not None}


# ================================================================== graph capture
def graphed_step_equals_eager(precision, image_size):
    """GraphedTrainStep on the key-tiled kernels (their torch-allocated workspaces inside the capture): the replays give the eager
    steps' losses and parameters bit for bit, as tests/test_train_gpu.py checks at 224^2."""
    from myrtle_vision.hip.functional import cross_entropy
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.graph import GraphedTrainStep
    from myrtle_vision.utils.optim import AdamW, ParamArena
    from myrtle_vision.utils.utils import seed_everything
    kw = dict(decoder="classification", num_classes=10, image_size=image_size, patch_size=16, dim=128, depth=2, heads=2,
              mlp_dim=256, dropout=0.0, emb_dropout=0.0)

    def loss_fn(m, x, y):
        return cross_entropy(m(x), y)

    gen = g(9)
    batches = [(torch.randn(4, 3, image_size, image_size, generator=gen).cuda(), torch.randint(0, 10, (4,), generator=gen).cuda())
               for _ in range(4)]
    lrs = [1e-3, 1e-3, 4e-4, 7e-4]

    def build():
        seed_everything(21)
        vit = ViT(precision=precision, q_format="FP32", **kw).cuda().train()
        opt = AdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05)
        opt.max_grad_norm = 1.0
        return vit, opt

    def set_lr(opt, lr):
        for grp in opt.param_groups:
            grp["lr"] = lr

    vit_e, opt_e = build()
    losses_e = []
    for i in [0, 0, 0, 1, 2, 3]:
        set_lr(opt_e, lrs[i])
        opt_e.zero_grad()
        loss = loss_fn(vit_e, *batches[i])
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss))
    vit_g, opt_g = build()
    graphed = GraphedTrainStep(vit_g, opt_g, loss_fn, *batches[0], warmup=3)
    losses_g = []
    for i in (1, 2, 3):
        set_lr(opt_g, lrs[i])
        losses_g.append(float(graphed(*batches[i])))
    torch.cuda.synchronize()
    assert opt_g.step_count == opt_e.step_count == 6
    assert losses_g == losses_e[3:]
    assert torch.equal(opt_g.arena.flat_param, opt_e.arena.flat_param)


# ================================================================== the tests every family repeats
def check_short_lengths_keep_the_whole_head_kernels(fam, ops, B, N, H, seed):
    """N <= cap still takes the whole-head kernels: the dispatching wrappers give exactly their bits, and the whole-head entry
    points keep their cap."""
    from myrtle_vision.hip.lib import lib
    assert fam.dh == 64                                 # the whole-head entry points take no width
    qkv, dout = make(fam, ops, B, N, H, seed=seed)
    qkv, dout = qkv.cuda(), dout.cuda()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty(B, N, H * fam.dh, dtype=torch.bfloat16 if fam.arith == "bf16" else torch.float32, device="cuda")
    lse = torch.empty(B, H, N, device="cuda")
    entry = getattr(lib(), fam.whole_head)
    assert entry(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), B, N, H, fam.scale, st) == 0
    torch.cuda.synchronize()
    out_d, lse_d = fam.forward(ops)(qkv, B, N, H, fam.scale)
    assert torch.equal(out_d, out) and torch.equal(lse_d, lse)
    assert entry(qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), 1, fam.cap + 1, 1, fam.scale, st) != 0
    if fam.arith == "fp32":                             # and the backward
        dqkv = fam.backward(ops)(qkv, out, dout, lse, B, N, H, fam.scale)
        d2 = torch.empty_like(qkv)
        assert lib().mv_attention_bwd_f32(qkv.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), d2.data_ptr(), B, N, H,
                                          fam.scale, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(dqkv, d2)
    torch.cuda.synchronize()


def check_deterministic(fam, ops):
    """Two runs give the same bits: out, lse, dqkv (half: the bf16 pieces of the split form) and the column sums."""
    B, N, H = 2, 1025, 3
    qkv, dout = make(fam, ops, B, N, H, seed=11)
    qkv, dout = qkv.cuda(), dout.cuda()
    fwd, bwd = fam.forward(ops), fam.backward(ops)
    runs = []
    for _ in range(2):
        out, lse = fwd(qkv, B, N, H, fam.scale)
        part = torch.empty(B, 3 * H * fam.dh, device="cuda")
        if fam.arith == "half":
            with ops.segments(3):
                dqkv = bwd(qkv, out, dout, lse, B, N, H, fam.scale, split=True, colsum=part)
        else:
            dqkv = bwd(qkv, out, dout, lse, B, N, H, fam.scale, colsum=part)
        runs.append((out, lse, dqkv, part))
    for a, b in zip(*runs):
        assert same_bits(a, b) and not bool(a.isnan().any())


def check_key_permutation(fam, ops):
    """Permuting keys and values together leaves softmax(QK^T)V, the lse and dQ unchanged up to the order of the fp32 sums and the
    rounding of P (which sees other running maxima); dK and dV permute with them."""
    bars = fam.bars
    B, N, H = 2, 577, 2
    qkv, dout = make(fam, ops, B, N, H, seed=13)
    qkv, dout = qkv.cuda(), dout.cuda()
    perm = torch.randperm(N, generator=g(14)).cuda()
    qkvp = permute_keys(qkv, perm, H, fam.dh)
    fwd, bwd = fam.forward(ops), fam.backward(ops)
    out, lse = fwd(qkv, B, N, H, fam.scale)
    out_p, lse_p = fwd(qkvp, B, N, H, fam.scale)
    assert relerr(out_p, out) < bars["perm_out"]
    assert float((lse_p - lse).abs().max()) < bars["perm_lse"]
    d = bwd(qkv, out, dout, lse, B, N, H, fam.scale).view(B, N, 3, H, fam.dh)
    dp = bwd(qkvp, out_p, dout, lse_p, B, N, H, fam.scale).view(B, N, 3, H, fam.dh)
    assert relerr(dp[:, :, 0], d[:, :, 0]) < bars["perm_grad"]
    for i in (1, 2):
        assert relerr(dp[:, :, i], d[:, perm, i]) < bars["perm_grad"], "kv"[i - 1]


def peak_growth(run):
    """-> (run(), the growth of the allocator's peak over what was allocated before)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = run()
    torch.cuda.synchronize()
    return r, torch.cuda.max_memory_allocated() - base


def check_no_n_squared_tensor(fam, ops, B, H, N):
    """Forward + backward allocate less than 1 / fam.n2_fraction of one [B, H, N, N] fp32 tensor; the materialised path holds the
    probabilities and a dP of that size."""
    from myrtle_vision.hip import functional as F
    assert B * H * N * N * 4 >= 256 * 2 ** 20
    bar = B * H * N * N * 4 / fam.n2_fraction
    qkv, dout = make(fam, ops, B, N, H, seed=17)
    dout = dout.cuda()
    if fam.arith == "half":                             # half q/k/v exist inside the bf16x3h block only: the wrappers, one by one
        part = torch.empty(B, 3 * H * fam.dh, device="cuda")
        (out, lse), grew_fwd = peak_growth(lambda: fam.forward(ops)(qkv, B, N, H, fam.scale))
        dqkv, grew_bwd = peak_growth(lambda: fam.backward(ops)(qkv, out, dout, lse, B, N, H, fam.scale, colsum=part))
        assert bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(part).all())
        assert grew_fwd < bar and grew_bwd < bar, (grew_fwd, grew_bwd, bar)
        return
    qkv = qkv.cuda().requires_grad_(True)

    def step():
        out = F.attention_core(qkv, H, fam.scale)
        out.backward(dout)
        return out

    out, grew = peak_growth(step)
    assert qkv.grad is not None and bool(torch.isfinite(qkv.grad.float()).all())
    # the results the call has to leave behind (out and qkv.grad) are not what this test is about, and at dh = 128 they alone are
    # larger than the bar (8 dh = 1 024 > N = 577 bytes per (image, head, token)): everything else must stay below it
    results = out.numel() * out.element_size() + qkv.grad.numel() * qkv.grad.element_size()
    print(f"{fam.name}: peak growth {grew} B, of which results {results} B; 1/{fam.n2_fraction} of [B, H, N, N] fp32 = {bar:.0f} B")
    assert grew - results < bar, (grew, results)
    if 8 * fam.dh < N:
        assert grew < bar, (grew, bar)                  # where the results fit under the bar: all of it


# ---------------------------------------------------------------- models
DH_MODELS = {32: dict(dim=192, heads=6, dim_head=32, depth=2, mlp_dim=768),           # the golden fixtures' micro widths
             128: dict(dim=384, heads=3, dim_head=128, depth=2, mlp_dim=1536)}        # ViT-Small's widths
CLS_384, SEG_512 = ("classification", 384, 45, "long_cls_384"), ("segmentation", 512, 17, "long_seg_512")
# what ops must (not) do while the model runs: every block's attention on the family's key-tiled kernels, no fall-back
WATCH = {"bf16": dict(),
         "half": dict(count=("attention_fwd_long_f16",), forbid_probs=True),
         "fp32": dict(attn_long=True, forbid_probs=True),
         "dh32": dict(attn_long=True, count=("attention_fwd_dh", "attention_bwd_dh")),
         "dh128": dict(attn_long=True, count=("attention_fwd_dh", "attention_bwd_dh"))}


def assert_long_vs_materialised(bars, tag, long, mat):
    (logits, grads), (logits_m, grads_m) = long, mat
    err = float((logits - logits_m).abs().max() / logits_m.abs().max())
    assert set(grads) == set(grads_m) and len(grads_m) > 20
    worst = max(relerr(grads[k], grads_m[k]) for k in grads_m)
    print(f"{tag}: vs materialised path: logits {err:.3e}, worst gradient {worst:.3e}")
    assert err < bars["mat_logits"], err
    assert worst < bars["mat_grad"], worst
    return err, worst


def check_model_matches_oracle(fam, ops, precision, decoder, image_size, num_classes, case):
    """A two-block model against the CPU oracle at the precision's contract (model_logits on the logits by max |logit|, model_grad
    relative L2 on every gradient tensor: the bf16 envelope, or the north-star bar of bf16x3h / fp32 / bf16x3), every block's
    attention on the family's key-tiled kernels.  The widths 32 and 128 also against the same model on the materialised path
    (``ops.ATTN_LONG`` off: what these widths took before)."""
    bars, name = fam.bars, fam.name
    cfg, kw, params, img, labels = model_case(decoder, image_size, num_classes, 2, case, DH_MODELS.get(fam.dh, MICRO))
    ref_logits, ref_loss, ref_grads = loss_and_grads(params, img, labels, cfg)
    with watching(ops, **WATCH[name]) as calls:
        vit = build_model(kw, precision, params)
        logits, grads = run_model(vit, img, labels)
    assert calls == {k: 2 for k in calls}                # both layers, forward and backward
    if name == "bf16":
        assert all(k in grads for k, _ in vit.named_parameters() if ref_grads[k] is not None)
    err, errs = model_errors(logits, grads, ref_logits, ref_grads)
    worst = max(errs.values())
    print(f"{case} {precision}: logits vs oracle {err:.3e}, worst gradient vs oracle {worst:.3e} over {len(errs)} tensors")
    if name == "fp32":
        report(f"attn_long_f32 {precision} {decoder} {image_size} logits vs oracle", err)
        report(f"attn_long_f32 {precision} {decoder} {image_size} worst gradient vs oracle", worst)
    assert err < bars["model_logits"], err
    for k, e in errs.items():
        assert e < bars["model_grad"], (k, e)
    assert len(errs) > 20
    if fam.long_fwd is None:
        with watching(ops, **dict(WATCH[name], attn_long=False)) as calls_m:
            mat = run_model(build_model(kw, precision, params), img, labels)
        assert calls_m == {k: 0 for k in calls}
        assert_long_vs_materialised(bars, case, (logits, grads), mat)


def vit_b_384(precision):
    """ViT-B/16 at 384^2 (577 tokens) in training mode, seeded"""
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.utils import seed_everything
    seed_everything(7)
    return ViT(precision=precision, q_format="FP32", decoder="classification", image_size=384, patch_size=16, num_classes=1000,
               dim=768, depth=12, heads=12, mlp_dim=3072, dropout=0.0, emb_dropout=0.0).cuda().train()
