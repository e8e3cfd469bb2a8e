"""Autograd functions of the ViT hot path on the HIP kernels.

Granular functions (``layer_norm``, ``linear``, ``gelu``, ``attention_core``, ``patch_embed`` ...) mirror one
reference module each and compose freely (used when fake-quant stubs sit between modules, or when a submodule
is called on its own).  The fused functions ``attn_block`` / ``mlp_block`` implement one whole
``Residual(PreNorm(...))`` of the reference (vit.py:131-151) with everything fusable fused into GEMM epilogues:

    attn_block:  LN -> QKV GEMM(+bias) -> fused attention -> proj GEMM(+bias +residual)
    mlp_block :  LN -> fc1 GEMM(+bias, GELU, keeps pre-activation) -> fc2 GEMM(+bias +residual)
    backward  :  dX GEMMs (fc2's with the GELU' epilogue), dW GEMMs (transposed LDS reads, split-K),
                 attention backward, LN backward with the residual gradient folded in.

Both blocks stand in one frame, written once: ``_block_open`` (up to the LayerNorm forward), ``_block_close`` (the closing product,
residual or drop-path add, the link to the next block), ``_block_grad_in`` (the incoming gradient) and ``_block_ln_bwd``.
``_AttnBlock`` / ``_MlpBlock`` hold only what lies between, once per arithmetic (split-operand or plain).

The residual stream and all gradients w.r.t. parameters are fp32; activations are bf16 (``prec='bf16'``) or fp32
(``prec='fp32'``: parity mode, fp32-accurate arithmetic).  Backward runs on autograd's worker thread: everything here is stateless
apart from caches keyed by tensor identity.
"""
import functools
import weakref

import torch
from torch.autograd import Function

from . import ops
from .ops import (EPI_DGELU, EPI_EMBED, EPI_GELU, EPI_GELU_GRAD, EPI_GELU_GRAD8, EPI_MUL, EPI_MUL8, EPI_NONE,
                  EPI_RESIDUAL)


GELU_GRAD_BITS = 8          # 8 | 16: width of the gelu'(h) the bf16 MLP block keeps for its backward pass


def _c(t):
    return t if t.is_contiguous() else t.contiguous()


def _scoped(backward):
    """Run one backward function inside ``ops.split_scope()``: its dX and dW products share the bf16x6 split of dY (fp32
    mode; a no-op for the bf16 path) -- and with the segment count its forward ran under (``_fwd``: 6 = bf16x6, 3 = bf16x3;
    backward runs on autograd's worker threads, which do not see the caller's thread-local scope)."""
    @functools.wraps(backward)
    def run(ctx, *args, **kwargs):
        with ops.split_scope(), ops.segments(getattr(ctx, "mv_segments", 6)):
            return backward(ctx, *args, **kwargs)
    return run


def _fwd(forward):
    """Forward of an autograd function that may hold fp32 Linear products: remember the segment count of the calling scope."""
    @functools.wraps(forward)
    def run(ctx, *args, **kwargs):
        # fused functions receive the model's precision as their last argument and follow it; granular ones (one reference
        # module each, no precision argument) follow the scope their caller opened (ViT.forward)
        # (the block functions take one more argument after it, the optional per-sample scale: a tensor or None)
        prec = next((a for a in reversed(args[-2:]) if isinstance(a, str)), None)
        ctx.mv_segments = ops.prec_segments(prec) if prec is not None else getattr(ops._seg_tls, "n", 6)
        with ops.segments(ctx.mv_segments):
            return forward(ctx, *args, **kwargs)
    return run


# ------------------------------------------------------------------------------------------------------------
# granular functions
# ------------------------------------------------------------------------------------------------------------
class _LayerNorm(Function):
    """nn.LayerNorm over the last dim (vit.py:37).  Input fp32 (any leading shape), output ``out_dtype``."""

    @staticmethod
    @_fwd
    def forward(ctx, x, gamma, beta, out_dtype, eps):
        ops.require_cuda(x, gamma, beta)
        x = _c(x.float())
        dim = x.shape[-1]
        rows = x.numel() // dim
        y, mean, rstd = ops.layernorm_fwd(x, dim, rows, dim, gamma, beta, out_dtype, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.beta = beta
        return y.view(x.shape)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dim = x.shape[-1]
        rows = x.numel() // dim
        dy = _c(dy)
        dx = torch.empty_like(x)
        dg, db = ops.layernorm_bwd(dy, x, dim, gamma, mean, rstd, None, dx, dim, rows, dim, beta=ctx.beta)
        return dx, dg, db, None, None


def layer_norm(x, gamma, beta, out_dtype=torch.float32, eps=1e-5):
    return _LayerNorm.apply(x, gamma, beta, out_dtype, eps)


class _Linear(Function):
    """nn.Linear: y = x W^T + b (vit.py:72,74,48,51,220,333).  x dtype selects the kernel family."""

    @staticmethod
    @_fwd
    def forward(ctx, x, weight, bias, out_dtype):
        ops.require_cuda(x, weight, bias)
        K = x.shape[-1]
        N = weight.shape[0]
        x2 = _c(x).view(-1, K)
        M = x2.shape[0]
        if x2.dtype == torch.bfloat16 and K % 8 != 0:
            raise RuntimeError(f"bf16 Linear needs in_features % 8 == 0 (got {K}); use precision='fp32'")
        out = torch.empty(M, N, dtype=out_dtype, device=x.device)
        ops.linear_fwd(x2, M, K, weight, bias, out, N)
        ctx.save_for_backward(x2, weight)
        ctx.has_bias = bias is not None
        ctx.bias = bias
        ctx.in_shape = x.shape
        return out.view(*x.shape[:-1], N)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        x2, weight = ctx.saved_tensors
        M, K = x2.shape
        N = weight.shape[0]
        dy2 = _c(dy).view(M, N)
        if dy2.dtype != x2.dtype:
            dy2 = ops.cast(dy2, x2.dtype)
        ld_dy = N
        if dy2.dtype == torch.bfloat16 and N % 8 != 0:      # pad the contraction dim of dX / rows of dW^T with zeros
            ld_dy = ops.pad8(N)
            padded = torch.zeros(M, ld_dy, dtype=dy2.dtype, device=dy2.device)
            padded[:, :N] = dy2
            dy2 = padded
        # dW first: in fp32 mode its split of dY also leaves the bias gradient, and the dX product below reuses that split
        dw, db = ops.linear_dw(dy2, x2, M, N, K, ld_dy=ld_dy, want_bias=ctx.has_bias, weight=weight, bias=ctx.bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=x2.dtype, device=x2.device)
            ops.linear_dx(dy2, M, N, weight, dx, K, ld_dy=ld_dy)
            dx = dx.view(ctx.in_shape)
        return dx, dw, db, None


def linear(x, weight, bias, out_dtype=None):
    return _Linear.apply(x, weight, bias, x.dtype if out_dtype is None else out_dtype)


class _LinearQatF16(Function):
    """nn.qat.Linear of the FP16 formats (utils/quantize.py:253-327) when its input already holds float_quantize(5, 10)
    values: y = x W_q^T + b with W_q = weight_fake_quant(W).  Both operands are exactly representable in IEEE half, so the
    forward product runs on the f16 matrix cores with fp32 accumulation -- the same numbers as the reference's fp32 GEMM of
    the same values up to summation order.  Backward is the straight-through estimator's: dX = dY W_q, dW = dY^T x in fp32
    (dY is not quantised, so those products stay on the f32 MFMA)."""

    @staticmethod
    @_fwd
    def forward(ctx, x, weight, bias):
        ops.require_cuda(x, weight, bias)
        K, N = x.shape[-1], weight.shape[0]
        x2 = _c(x.float()).view(-1, K)
        M = x2.shape[0]
        x16 = ops.quant_float_f16(x2)                          # idempotent on already-quantised values: an exact conversion
        w16 = ops.quant_float_f16(weight)                      # weight_fake_quant and the half conversion in one pass
        out = torch.empty(M, N, dtype=torch.float32, device=x.device)
        ops.linear_f16(x16, w16, M, N, K, bias, out)
        ctx.save_for_backward(x2, ops.quant_float(weight, 5, 10))
        ctx.params = (weight, bias)
        ctx.in_shape = x.shape
        return out.view(*x.shape[:-1], N)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        x2, wq = ctx.saved_tensors
        weight, bias = ctx.params
        M, K = x2.shape
        N = wq.shape[0]
        dy2 = _c(dy.float()).view(M, N)
        dw, db = ops.linear_dw(dy2, x2, M, N, K, want_bias=bias is not None, weight=weight, bias=bias)   # dW first: see _Linear
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, dtype=torch.float32, device=dy.device)
            ops.linear_dx(dy2, M, N, wq, dx, K)
            dx = dx.view(ctx.in_shape)
        return dx, dw, db


def linear_qat_f16(x, weight, bias):
    return _LinearQatF16.apply(x, weight, bias)


class _Gelu(Function):
    @staticmethod
    @_fwd
    def forward(ctx, x):
        ops.require_cuda(x)
        x = _c(x)
        ctx.save_for_backward(x)
        return ops.gelu_fwd(x)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = _c(dy)
        if dy.dtype != x.dtype:
            dy = ops.cast(dy, x.dtype)
        return ops.gelu_bwd(x, dy)


def gelu(x):
    return _Gelu.apply(x)


class _Cast(Function):
    @staticmethod
    @_fwd
    def forward(ctx, x, dtype):
        ctx.src_dtype = x.dtype
        return ops.cast(_c(x), dtype)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        return ops.cast(_c(dy), ctx.src_dtype), None


def cast(x, dtype):
    return x if x.dtype == dtype else _Cast.apply(x, dtype)


class _Add(Function):
    """FloatFunctional.add of the residual (vit.py:27) in the unfused path."""

    @staticmethod
    @_fwd
    def forward(ctx, a, b):
        ops.require_cuda(a, b)
        return ops.add_f32(_c(a.float()), _c(b.float()))

    @staticmethod
    @_scoped
    def backward(ctx, d):
        return d, d


def add(a, b):
    return _Add.apply(a, b)


class _Dropout(Function):
    """nn.Dropout(p) in training mode (vit.py:50,52,75,311).  The mask is a function of (seed, offset) drawn from torch's
    CPU generator in forward -- reproducible under ``seed_everything`` -- and regenerated in backward, never stored."""

    @staticmethod
    @_fwd
    def forward(ctx, x, p):
        ops.require_cuda(x)
        seed, offset = (int(v) for v in torch.randint(0, 2 ** 62, (2,), dtype=torch.int64).tolist())
        ctx.rng = (float(p), seed, offset)
        return ops.dropout(_c(x), p, seed, offset)

    @staticmethod
    @_scoped
    def backward(ctx, dy):
        p, seed, offset = ctx.rng
        return ops.dropout(_c(dy), p, seed, offset), None


def dropout(x, p, training=True):
    if p == 0.0 or not training:
        return x
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability has to be in [0, 1), got {p}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    return _Dropout.apply(x, p)


class _AttentionFused(Function):
    """softmax(q k^T * scale) v on the fused kernels of one ``ops.attention_path`` (any but the materialised one; no [B, H, N, N]
    tensor): saves qkv, out and the log-sum-exp, the backward kernels recompute the probabilities.  qkv [B, N, 3*H*dh] ->
    [B, N, H*dh] in qkv's dtype.  The decorators are for the Linear products of other functions: no attention kernel on these
    paths reads the split memo or the segment count."""

    @staticmethod
    @_fwd
    def forward(ctx, path, qkv, heads, scale):
        B, N, three_d = qkv.shape
        qkv = _c(qkv)
        dh = three_d // (3 * heads)
        out, lse = ops.attention_forward(path, qkv, B, N, heads, dh, scale)
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (path, heads, dh, scale)
        return out

    @staticmethod
    @_scoped
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        path, heads, dh, scale = ctx.cfg
        B, N, _ = qkv.shape
        if qkv.dtype == torch.bfloat16:                  # the kernels read dO in q/k/v's format
            dout = _c(dout)
            if dout.dtype != torch.bfloat16:
                dout = ops.cast(dout, torch.bfloat16)
        else:
            dout = _c(dout.float())
        return None, ops.attention_backward(path, qkv, out, dout, lse, B, N, heads, dh, scale), None, None


class _AttentionProbs(Function):
    """Materialised fp32 path, part 1: probs = softmax(q k^T * scale)  [B, H, N, N] (vit.py:92-93)."""

    @staticmethod
    @_fwd
    def forward(ctx, qkv, heads, scale):
        B, N, three_d = qkv.shape
        dh = three_d // (3 * heads)
        qkv = _c(qkv)
        probs = ops.attention_probs_fp32(qkv, B, N, heads, dh, scale)
        ctx.save_for_backward(qkv, probs)
        ctx.heads, ctx.scale, ctx.dh = heads, scale, dh
        return probs

    @staticmethod
    @_scoped
    def backward(ctx, dprobs):
        qkv, probs = ctx.saved_tensors
        B, N, _ = qkv.shape
        H, dh, D = ctx.heads, ctx.dh, ctx.heads * ctx.dh
        L = ops.lib()
        dS = torch.empty_like(probs)
        dprobs = _c(dprobs)
        ops.check(L.mv_softmax_bwd(probs.data_ptr(), dprobs.data_ptr(), dS.data_ptr(), B * H * N, N, ctx.scale, ops._s()),
                  "softmax_bwd")
        dqkv = torch.zeros_like(qkv)
        flat, dflat = qkv.view(-1), dqkv.view(-1)
        bq, hq, bp, hp = N * 3 * D, dh, H * N * N, N * N
        ops.check(L.mv_gemm_f32(dS.data_ptr(), N, 1, bp, hp, flat[D:].data_ptr(), 3 * D, 1, bq, hq, dqkv.data_ptr(), 3 * D, 1,
                                bq, hq, N, dh, N, B, H, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, ops._s()), "gemm_f32(dQ)")
        ops.check(L.mv_gemm_f32(dS.data_ptr(), 1, N, bp, hp, qkv.data_ptr(), 3 * D, 1, bq, hq, dflat[D:].data_ptr(), 3 * D, 1,
                                bq, hq, N, dh, N, B, H, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, ops._s()), "gemm_f32(dK)")
        return dqkv, None, None


class _AttentionPV(Function):
    """Materialised fp32 path, part 2: out = (probs @ v).transpose(1,2).reshape(B,N,C) (vit.py:96)."""

    @staticmethod
    @_fwd
    def forward(ctx, probs, qkv, heads):
        B, N, three_d = qkv.shape
        dh = three_d // (3 * heads)
        probs, qkv = _c(probs), _c(qkv)
        ctx.save_for_backward(probs, qkv)
        ctx.heads, ctx.dh = heads, dh
        return ops.attention_pv_fp32(probs, qkv, B, N, heads, dh)

    @staticmethod
    @_scoped
    def backward(ctx, dout):
        probs, qkv = ctx.saved_tensors
        B, N, _ = qkv.shape
        H, dh, D = ctx.heads, ctx.dh, ctx.heads * ctx.dh
        L = ops.lib()
        dout = _c(dout.float())
        flat = qkv.view(-1)
        bq, hq, bp, hp, bo, ho = N * 3 * D, dh, H * N * N, N * N, N * D, dh
        dP = torch.empty_like(probs)
        ops.check(L.mv_gemm_f32(dout.data_ptr(), D, 1, bo, ho, flat[2 * D:].data_ptr(), 1, 3 * D, bq, hq, dP.data_ptr(), N, 1,
                                bp, hp, N, N, dh, B, H, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, ops._s()), "gemm_f32(dP)")
        dqkv = torch.zeros_like(qkv)
        ops.check(L.mv_gemm_f32(probs.data_ptr(), 1, N, bp, hp, dout.data_ptr(), D, 1, bo, ho,
                                dqkv.view(-1)[2 * D:].data_ptr(), 3 * D, 1, bq, hq, N, dh, N, B, H, 1.0, 0, None, EPI_NONE,
                                None, 0, 0, None, 0, ops._s()), "gemm_f32(dV)")
        return dP, dqkv, None


def attention_core(qkv, heads, scale, probs_hook=None):
    """Attention.forward lines vit.py:87-96 on a to_qkv output [B, N, 3*heads*dh].

    ``probs_hook`` (callable or None) is the reference's ``attn_output`` Identity (vit.py:80-82,94): when it has
    forward hooks the probabilities are materialised (fp32) and passed through it; otherwise bf16 inputs take the
    fused kernels (head widths 64, 32 and 128)."""
    B, N, three_d = qkv.shape
    dh = three_d // (3 * heads)
    path = ops.attention_path(qkv.dtype, N, dh, need_grad=torch.is_grad_enabled() and qkv.requires_grad,
                              hook=probs_hook is not None)
    if path != ops.ATTN_PROBS:
        return _AttentionFused.apply(path, qkv, heads, scale)
    src_dtype = qkv.dtype
    q32 = cast(qkv, torch.float32)
    probs = _AttentionProbs.apply(q32, heads, scale)
    if probs_hook is not None:
        probs = probs_hook(probs)
    out = _AttentionPV.apply(probs, q32, heads)
    return cast(out, src_dtype)


class _PatchEmbed(Function):
    """patchify + patch_to_embedding + cls token + positional embedding (vit.py:271-311) -> fp32 [B, T, D]."""

    @staticmethod
    @_fwd
    def forward(ctx, img, weight, bias, cls_token, pos, patch, prec):
        ops.require_cuda(img, weight, bias, cls_token, pos)
        adt = ops.act_dtype(prec)
        B, C, H, W = img.shape
        npatch = (H // patch) * (W // patch)
        T, D, pd = npatch + 1, weight.shape[0], weight.shape[1]
        if adt == torch.bfloat16 and pd % 8 != 0:
            raise RuntimeError(f"bf16 patch embedding needs patch_dim % 8 == 0 (got {pd}); use precision='fp32'")
        patches = ops.patchify(img, patch, adt)
        x = torch.empty(B, T, D, dtype=torch.float32, device=img.device)
        pos2 = _c(pos.detach().float()).view(T, D)
        ops.linear_fwd(patches, B * npatch, pd, weight, bias, x, D, epi=EPI_EMBED, aux=pos2, ld_aux=D, aux_i=npatch)
        ops.embed_cls(_c(cls_token.detach()).view(D), pos2, x, B, T, D)
        ctx.save_for_backward(patches)
        ctx.dims = (B, T, D, pd, npatch)
        ctx.pos_shape, ctx.cls_shape = pos.shape, cls_token.shape
        ctx.params = (weight, bias, cls_token, pos if pos.shape[-2:] == (T, D) and pos.is_leaf else None)
        chain_reset()
        return x

    @staticmethod
    @_scoped
    def backward(ctx, dx):
        (patches,) = ctx.saved_tensors
        B, T, D, pd, npatch = ctx.dims
        dx = _c(dx.float())
        weight, bias, cls_token, pos = ctx.params
        dpos, dcls, dy = ops.embed_bwd_gather(dx, B, T, D, patches.dtype, pos=pos, cls_token=cls_token)   # one pass over dx
        dw, db = ops.linear_dw(dy, patches, B * npatch, D, pd, weight=weight, bias=bias)
        return None, dw, db, dcls.view(ctx.cls_shape), dpos.view(ctx.pos_shape), None, None


def patch_embed(img, weight, bias, cls_token, pos, patch, prec):
    if img.requires_grad:
        raise RuntimeError("gradient w.r.t. the input image is not implemented (the reference never needs it)")
    return _PatchEmbed.apply(img, weight, bias, cls_token, pos, patch, prec)


class _PosResize(Function):
    """cls slot + the (sh, sw) grid of the positional embedding bicubically resized to (gh, gw) (vit.py:292-302) -> fp32
    [1, 1 + gh*gw, D].  The backward writes the parameter's gradient into its arena slot when it has one (``ops.grad_out``)."""

    @staticmethod
    def forward(ctx, pos, gh, gw, sh, sw):
        ops.require_cuda(pos)
        D = pos.shape[-1]
        ctx.dims = (gh, gw, sh, sw, D)
        ctx.pos_shape = pos.shape
        ctx.param = pos if pos.is_leaf else None
        return ops.pos_resize_fwd(ops._f32c(pos).view(1 + sh * sw, D), gh, gw, sh, sw).view(1, 1 + gh * gw, D)

    @staticmethod
    def backward(ctx, dout):
        gh, gw, sh, sw, D = ctx.dims
        dpos = ops.pos_resize_bwd(_c(dout.float()).view(1 + gh * gw, D), gh, gw, param=ctx.param, sh=sh, sw=sw)
        return dpos.view(ctx.pos_shape), None, None, None, None


def pos_resize(pos_embedding, gh, gw, sh=14, sw=14):
    """``pos_embedding`` [1, 1 + sh*sw, D] (or [1 + sh*sw, D]) -> [1, 1 + gh*gw, D]; needs ``ops.pos_resize_supported(D, gh, gw, sh, sw)``."""
    if pos_embedding.shape[-2] != 1 + sh * sw:
        raise ValueError(f"expected 1 + {sh}*{sw} rows, got {tuple(pos_embedding.shape)}")
    return _PosResize.apply(pos_embedding, gh, gw, sh, sw)


# ------------------------------------------------------------------------------------------------------------
# fused transformer blocks
# ------------------------------------------------------------------------------------------------------------
# One-slot side channel along the backward chain: the LayerNorm-backward kernel that produces a block's input
# gradient dx can also emit (a) dx in bf16 and (b) its column sums -- exactly what the NEXT block function to run
# (the one whose output gradient is this dx) needs as MFMA operand and as output-projection bias gradient.  Keeping
# a strong reference to dx pins its address, so a pointer match identifies the tensor unambiguously.
# Each entry carries its KIND: "bf16" (dx16, the [rows, dim] bf16 copy of dx) or ("split", nseg) (the [rows, nseg * dim] bf16
# pieces of dx).  Precision is per block, so producer and consumer may run different arithmetics: a consumer takes only the kind
# it reads (a bf16 block in front of an fp32 one must not read the latter's pieces as its dY) and otherwise computes its own.
_side = {}


def _publish_side(dx, side, colsum, kind):
    _side.clear()
    _side[dx.data_ptr()] = (dx, side, colsum, kind)


def _take_side(dout, rows, dim, kind):
    """(side tensor, column sums) published for ``dout`` if it is of ``kind`` ("bf16" or ("split", nseg)), else (None, None)."""
    ent = _side.pop(dout.data_ptr(), None)
    _side.clear()
    width = dim if kind == "bf16" else kind[1] * dim
    if ent is None or ent[3] != kind or ent[0].shape != dout.shape or tuple(ent[1].shape) != (rows, width):
        return None, None
    return ent[1], ent[2]


def _ln_bwd_with_side(dy, x, D, g, b, mean, rstd, dout, M, adt, up_bias=None):
    """LayerNorm backward + residual gradient; in bf16 mode also publishes the bf16 copy and column sums of dx.
    ``up_bias``: the bias of the Linear that produced x (recorded in forward, ``_chain``): the column sums ARE its
    gradient, so they are written straight to its destination."""
    dx = torch.empty_like(x)
    if adt == torch.bfloat16:
        dx16 = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
        cs = ops.grad_out(up_bias, (D,), x.device)
        dg, db = ops.layernorm_bwd(dy, x, D, g, mean, rstd, dout, dx, D, M, D, dx16=dx16, dx_colsum=cs, beta=b)
        _publish_side(dx, dx16, cs, "bf16")
    elif D <= 1024 and ops.x6_block_ok(M, D):
        # split-operand modes: dx also leaves as the pieces the consumer's dW / dX products read, with its column sums (that Linear's
        # bias gradient): the consumer (the block before this one, _take_side) then needs no split pass over dx
        dx6 = ops._split_buffer(M, D, x.device)
        cs = ops.grad_out(up_bias, (D,), x.device)
        dg, db = ops.layernorm_bwd(dy, x, D, g, mean, rstd, dout, dx, D, M, D, dx_split=dx6, dx_colsum=cs, beta=b)
        _publish_side(dx, dx6, cs, ("split", ops.current_segments()))
    else:
        dg, db = ops.layernorm_bwd(dy, x, D, g, mean, rstd, dout, dx, D, M, D, beta=b)
    return dx, dg, db


# Forward-order link between consecutive block functions: (the tensor OBJECT a block returned, held weakly, and the bias of
# the Linear that produced it).  The next block reads it to learn whose bias gradient the column sums of its dx are.
# Identity, not address: a freed-and-reallocated buffer at the same address can never inherit the link.
_chain = [None]


def _chain_set(out, bias):
    _chain[0] = (weakref.ref(out), bias) if bias is not None else None


def _chain_take(x):
    c = _chain[0]
    return c[1] if c is not None and c[0]() is x else None


def chain_reset():
    """Forget the link (start of a forward pass, or a block called on its own)."""
    _chain[0] = None


# Stochastic depth (drop path) on the fused blocks: out[b] = x[b] + c[b] * f(LN(x[b])) with one factor c[b] per sample (``row_scale``,
# fp32 [B]: 0 or 1 / (1 - p)).  Everything in a branch after its last non-linearity is linear, so the block keeps its fused path: the
# last product runs without the residual and ``ops.drop_path_add`` finishes the row; in backward the branch's incoming gradient is
# c * dout (``ops.row_scale``) and everything downstream of it is unchanged, while the residual gradient stays the unscaled dout:
# dx = dout + LNbwd(J^T (c * dout)).  Two hand-offs between neighbouring blocks assume c == 1 and are switched off for such a block:
# the forward link (``_chain_set(out, None)``: the next block's LayerNorm backward would write colsum(dout) into this block's
# output-bias gradient, which is colsum(c * dout)) and the published side (bf16(dout) and colsum(dout), both unscaled).  All of it
# lives in the frame below: ``_block_close`` (the product without the residual, the add, no link) and ``_block_grad_in`` (c * dout,
# no side); a block function never looks at ``row_scale``.
def _row_scale_arg(x, row_scale):
    if row_scale.dtype != torch.float32 or row_scale.dim() != 1 or row_scale.shape[0] != x.shape[0] or row_scale.requires_grad:
        raise ValueError(f"row_scale: expected an fp32 [{x.shape[0]}] tensor without gradient, got {tuple(row_scale.shape)} "
                         f"{row_scale.dtype}")
    ops.require_cuda(row_scale)
    return _c(row_scale)


# The frame both fused blocks share: out = x + c * last(f(LN(x))), ``last`` being the block's closing Linear.  A block function states f and
# its gradient, once per arithmetic: split-operand (``ctx.x6``: fp32, bf16x3, bf16x3h with every product of the block on the bf16x6 / x3
# kernels; activations travel as their bf16 pieces [M, nseg * cols]) or plain (bf16, fp32 without ``x6_block_ok``; activations in ``ctx.adt``).
def _block_open(ctx, x, g, b, prec, row_scale, *widths):
    """Everything up to and including the LayerNorm forward -> (x contiguous, LN(x) as the operand the arithmetic reads -- ``adt``
    or pieces --, mean, rstd).  ``widths``: the block's feature widths besides D, for the ``x6_block_ok`` decision."""
    ctx.adt = adt = ops.act_dtype(prec)
    ctx.row_scale = row_scale
    B, T, D = x.shape
    M = B * T
    x = _c(x)
    ctx.up_bias = _chain_take(x)
    ctx.x6 = adt == torch.float32 and ops.x6_block_ok(M, D, *widths)
    if ctx.x6 and D <= 1024:
        y, mean, rstd = ops.layernorm_fwd_split(x, D, M, D, g, b)       # LayerNorm writes the pieces itself (no fp32 y, no split pass)
    else:
        y, mean, rstd = ops.layernorm_fwd(x, D, M, D, g, b, adt)
        if ctx.x6:
            y = ops.split_ex(y, M, D)
    return x, y, mean, rstd


def _block_close(ctx, a, weight, bias, x):
    """The closing product and the forward link: out = x + a W^T + bias in the GEMM's residual epilogue, or for a drop-path block
    the product without the residual and out = x + c * (a W^T + bias) by ``ops.drop_path_add``.  ``a``: [M, K] in ``adt``, or its pieces."""
    B, T, D = x.shape
    M, c = B * T, ctx.row_scale
    out = torch.empty_like(x)
    if ctx.x6:
        ops.nt_x6(a, weight, "fwd", M, out.view(M, D), bias=bias, residual=x.view(M, D) if c is None else None)
    elif c is None:
        ops.linear_fwd(a, M, weight.shape[1], weight, bias, out, D, epi=EPI_RESIDUAL, aux=x, ld_aux=D)
    else:
        ops.linear_fwd(a, M, weight.shape[1], weight, bias, out, D, epi=EPI_NONE)
    if c is not None:
        ops.drop_path_add(x, out, c)
    _chain_set(out, bias if c is None else None)
    return out


def _block_grad_in(ctx, dout, bias):
    """The gradient entering the closing Linear (dout, or c * dout for a drop-path block) as the operand the arithmetic reads, and
    that Linear's bias gradient -> (d, dbias).  Split-operand: the pieces, dbias always filled.  Plain: [M, D] in ``adt``; dbias is
    the column sums the producing LayerNorm backward published with the bf16 copy, or None: ``linear_dw`` computes it then."""
    B, T, D = dout.shape
    M, c = B * T, ctx.row_scale
    # first what the producing LayerNorm backward published for dout: plain fp32 has no side, and a drop-path block must not read it
    # (it is unscaled) and clears it
    if ctx.x6 or ctx.adt == torch.bfloat16:
        if c is None:
            d, dbias = _take_side(dout, M, D, ("split", ops.current_segments()) if ctx.x6 else "bf16")
            if d is not None:
                return d, dbias
        else:
            _side.clear()
    # else computed here; split-operand: one pass leaves the split and the bias gradient
    dbias = ops.grad_out(bias, (D,), dout.device) if ctx.x6 else None
    d = (ops.cast(dout, ctx.adt) if c is None else ops.row_scale(dout, c, ctx.adt)).view(M, D)
    return (ops.split_ex(d, M, D, colsum_out=dbias) if ctx.x6 else d), dbias


def _block_ln_bwd(ctx, dy, dout, x, g, b, mean, rstd):
    """The backward tail: LayerNorm backward of dy plus the residual gradient dout -> (dx, dgamma, dbeta), with the hand-off."""
    M, D = dy.shape
    return _ln_bwd_with_side(dy, x, D, g, b, mean, rstd, dout, M, ctx.adt, ctx.up_bias)


class _DropPath(Function):
    """y[b] * c[b] on the module-by-module path (timm's DropPath with the factors drawn elsewhere); same dtype out as in."""

    @staticmethod
    def forward(ctx, y, row_scale):
        ops.require_cuda(y, row_scale)
        ctx.save_for_backward(row_scale)
        return ops.row_scale(_c(y), row_scale)

    @staticmethod
    def backward(ctx, dy):
        (row_scale,) = ctx.saved_tensors
        return ops.row_scale(_c(dy), row_scale), None


def drop_path(y, row_scale):
    """c[b] * y[b] for y [B, ...] (fp32 or bf16) and the per-sample factors ``row_scale`` (fp32 [B]); None = identity."""
    if row_scale is None:
        return y
    return _DropPath.apply(y, _row_scale_arg(y, row_scale))


class _AttnBlock(Function):
    """x + to_out(attention(to_qkv(LN(x))))  ==  Residual(PreNorm(dim, Attention)) (vit.py:131-141, 84-99)."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, wqkv, bqkv, wo, bo, heads, scale, prec, row_scale=None):
        B, T, D = x.shape
        M = B * T
        inner3 = wqkv.shape[0]
        inner = inner3 // 3
        dh = inner // heads
        x, y, mean, rstd = _block_open(ctx, x, g, b, prec, row_scale, inner3, inner)
        adt, o6 = ctx.adt, None
        if ctx.x6:
            # every Linear product on the bf16x6 / x3 path: the block keeps the SPLITS of LN(x) and of the attention output (what the
            # forward and the dW products both read), not the tensors themselves
            ctx.path = path = ops.attention_path(adt, T, dh, need_grad=any(ctx.needs_input_grad), half_ok=True)
            # precision "bf16x3h": the fused attention kernels on half operands (2^-12 per rounding, fp32 sums, softmax and outputs);
            # q / k / v leave the to_qkv product as half (one rounding of the fp32 accumulator + bias, no fp32 tensor, no cast pass)
            qkv = torch.empty(B, T, inner3, dtype=torch.float16 if path == ops.ATTN_F16 else adt, device=x.device)
            ops.nt_x6(y, wqkv, "fwd", M, qkv.view(M, inner3), bias=bqkv)
            o, saved = ops.attention_forward(path, qkv, B, T, heads, dh, scale)
            o6 = ops.split_ex(o.view(M, inner), M, inner)
        else:
            qkv = torch.empty(B, T, inner3, dtype=adt, device=x.device)
            ops.linear_fwd(y, M, D, wqkv, bqkv, qkv, inner3)
            # half_ok stays off: q/k/v and dO are in ``adt`` here, so of ops.ATTN_COLSUM_PATHS only the two bf16 ones can come back
            ctx.path = path = ops.attention_path(adt, T, dh, need_grad=any(ctx.needs_input_grad))
            assert path != ops.ATTN_F16
            if path == ops.ATTN_PROBS:              # materialised fp32 probabilities (shapes the fused kernels lack)
                o, saved = ops.attention_forward(path, ops.cast(qkv, torch.float32), B, T, heads, dh, scale)
                o = ops.cast(o, adt)
            else:
                o, saved = ops.attention_forward(path, qkv, B, T, heads, dh, scale)
        out = _block_close(ctx, o6 if ctx.x6 else o.view(M, inner), wo, bo, x)
        # y: LN(x) in ``adt``, or its pieces; o6: the pieces of o (split-operand only; the fused backward needs o too: delta = rowsum(dO * O));
        # ``saved``: what ops.attention_forward returned on ctx.path: the log-sum-exp, the probabilities, or None (nothing runs backward then)
        ctx.save_for_backward(x, g, mean, rstd, y, qkv, None if ctx.x6 and path == ops.ATTN_PROBS else o, o6, saved, wqkv, wo)
        ctx.cfg = (heads, scale)
        ctx.small = (b, bqkv, bo)
        return out

    @staticmethod
    @_scoped
    def backward(ctx, dout):
        x, g, mean, rstd, y, qkv, o, o6, saved, wqkv, wo = ctx.saved_tensors
        heads, scale = ctx.cfg
        B, T, D = x.shape
        M = B * T
        inner3 = wqkv.shape[0]
        inner = inner3 // 3
        dh = inner // heads
        b, bqkv, bo = ctx.small
        adt = ctx.adt
        dout = _c(dout)
        d, dbo = _block_grad_in(ctx, dout, bo)                    # dY of the projection
        if ctx.x6:
            dwo = ops.tn_x6(d, o6, M, wo)
            do = torch.empty(B, T, inner, dtype=torch.float32, device=x.device)
            ops.nt_x6(d, wo, "dx", M, do.view(M, inner))
            dbqkv = ops.grad_out(bqkv, (inner3,), x.device)
            if ctx.path == ops.ATTN_F16:
                # the kernel writes the pieces of dqkv and per-image column sums itself: no fp32 dqkv, no split pass
                part = torch.empty(B, inner3, dtype=torch.float32, device=x.device)
                dq6 = ops.attention_backward(ctx.path, qkv, o, do, saved, B, T, heads, dh, scale, split=True, colsum=part)
                ops.colsum(part, B, inner3, inner3, dbqkv)
            else:
                dqkv = ops.attention_backward(ctx.path, qkv, o, do, saved, B, T, heads, dh, scale)
                dq6 = ops.split_ex(dqkv.view(M, inner3), M, inner3, colsum_out=dbqkv)
            dwqkv = ops.tn_x6(dq6, y, M, wqkv)
            dy = torch.empty(M, D, dtype=torch.float32, device=x.device)
            ops.nt_x6(dq6, wqkv, "dx", M, dy)
        else:
            # bf16: dW of to_out is computed below, with dW of to_qkv, in one grouped split-K launch (d and o stay alive)
            pair = adt == torch.bfloat16
            if not pair:
                dwo, dbo2 = ops.linear_dw(d, o.view(M, inner), M, D, inner, want_bias=dbo is None, weight=wo, bias=bo)
                dbo = dbo if dbo is not None else dbo2
            do = torch.empty(B, T, inner, dtype=adt, device=x.device)
            ops.linear_dx(d, M, D, wo, do, inner)
            dbqkv = None
            if ctx.path in ops.ATTN_COLSUM_PATHS:
                # the kernel also leaves per-image column sums of dqkv: to_qkv's bias gradient without another pass over dqkv
                part = torch.empty(B, inner3, dtype=torch.float32, device=x.device)
                dqkv = ops.attention_backward(ctx.path, qkv, o, do, saved, B, T, heads, dh, scale, colsum=part)
                dbqkv = ops.colsum(part, B, inner3, inner3, ops.grad_out(bqkv, (inner3,), x.device))
            elif ctx.path == ops.ATTN_PROBS:
                dqkv = ops.cast(ops.attention_backward(ctx.path, ops.cast(qkv, torch.float32), None, ops.cast(do, torch.float32), saved,
                                                       B, T, heads, dh, scale), adt)
            else:
                dqkv = ops.attention_backward(ctx.path, qkv, o, do, saved, B, T, heads, dh, scale)
            if pair:
                (dwo, dbo2), (dwqkv, dbq2) = ops.linear_dw_pair(M, (d, o.view(M, inner), D, inner, wo, bo, dbo is None),
                                                                (dqkv.view(M, inner3), y, inner3, D, wqkv, bqkv, dbqkv is None))
                dbo = dbo if dbo is not None else dbo2
            else:
                dwqkv, dbq2 = ops.linear_dw(dqkv.view(M, inner3), y, M, inner3, D, want_bias=dbqkv is None, weight=wqkv, bias=bqkv)
            dbqkv = dbqkv if dbqkv is not None else dbq2
            dy = torch.empty(M, D, dtype=adt, device=x.device)
            ops.linear_dx(dqkv.view(M, inner3), M, inner3, wqkv, dy, D)
        return (*_block_ln_bwd(ctx, dy, dout, x, g, b, mean, rstd), dwqkv, dbqkv, dwo, dbo, None, None, None, None)


def attn_block(x, g, b, wqkv, bqkv, wo, bo, heads, scale, prec, *, row_scale=None):
    """``row_scale`` (fp32 [B] on the device, or None): the drop-path factors c of this branch, out[b] = x[b] + c[b] * f(LN(x[b]))."""
    if row_scale is None:
        return _AttnBlock.apply(x, g, b, wqkv, bqkv, wo, bo, heads, scale, prec)
    return _AttnBlock.apply(x, g, b, wqkv, bqkv, wo, bo, heads, scale, prec, _row_scale_arg(x, row_scale))


class _MlpBlock(Function):
    """x + fc2(gelu(fc1(LN(x))))  ==  Residual(PreNorm(dim, FeedForward)) (vit.py:142-151, 44-56)."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, w1, b1, w2, b2, prec, row_scale=None):
        B, T, D = x.shape
        M = B * T
        Hd = w1.shape[0]
        x, y, mean, rstd = _block_open(ctx, x, g, b, prec, row_scale, Hd)
        adt = ctx.adt
        if ctx.x6:
            # keeps the splits of LN(x) and of gelu(h) plus the pre-activation h; the fp32 activation gelu(h) is never stored (the
            # split kernel applies the GELU on its way)
            h = torch.empty(M, Hd, dtype=adt, device=x.device)
            if ops.nt_split_ok(M, Hd, D):
                a = ops.nt_x6_gelu_split(y, w1, M, h, bias=b1)       # one launch: h (fp32) and the pieces of gelu(h)
            else:
                ops.nt_x6(y, w1, "fwd", M, h, bias=b1)
                a = ops.split_ex(h, M, Hd, op=1)
        else:
            # bf16: the fc1 epilogue leaves gelu'(pre-activation) for the backward pass (one multiply there instead of another
            # erf evaluation per element) -- as ONE BYTE per element (GELU_GRAD_BITS = 8: gelu' is confined to [-0.13, 1.13], a
            # 0.005-step code whose grid holds 0 and 1 exactly costs 0.24 % of its rms value and takes a quarter of the bytes out of fc1's store-bound epilogue
            # and of fc2-dX's); fp32 exact mode keeps the pre-activation itself
            g8 = adt == torch.bfloat16 and GELU_GRAD_BITS == 8 and Hd % 8 == 0
            h = torch.empty(M, Hd, dtype=torch.uint8 if g8 else adt, device=x.device)
            a = torch.empty(M, Hd, dtype=adt, device=x.device)
            ops.linear_fwd(y, M, D, w1, b1, a, Hd, epi=(EPI_GELU_GRAD8 if g8 else EPI_GELU_GRAD) if adt == torch.bfloat16 else EPI_GELU,
                           out2=h, ld_out2=Hd)
        out = _block_close(ctx, a, w2, b2, x)
        # y: LN(x), a: gelu(fc1) -- in ``adt``, or their pieces; h: fc1's pre-activation, or gelu' of it in the bf16 arithmetic
        ctx.save_for_backward(x, g, mean, rstd, y, h, a, w1, w2)
        ctx.small = (b, b1, b2)
        return out

    @staticmethod
    @_scoped
    def backward(ctx, dout):
        x, g, mean, rstd, y, h, a, w1, w2 = ctx.saved_tensors
        B, T, D = x.shape
        M = B * T
        Hd = w1.shape[0]
        b, b1, b2 = ctx.small
        adt = ctx.adt
        dout = _c(dout)
        d, db2 = _block_grad_in(ctx, dout, b2)                       # dY of fc2
        if ctx.x6:
            dw2 = ops.tn_x6(d, a, M, w2)
            db1 = ops.grad_out(b1, (Hd,), x.device)
            if ops.nt_split_ok(M, Hd, D):
                dh6 = ops.nt_x6_dgelu_split(d, w2, M, h, db1)    # one launch: the pieces of (dY W2) * gelu'(h) and its column sums
            else:
                dh = torch.empty(M, Hd, dtype=torch.float32, device=x.device)
                ops.nt_x6(d, w2, "dx", M, dh)
                dh6 = ops.split_ex(dh, M, Hd, op=2, h=h, colsum_out=db1)     # (dY W2) * gelu'(h), its split and its column sums
            dw1 = ops.tn_x6(dh6, y, M, w1)
            dy = torch.empty(M, D, dtype=torch.float32, device=x.device)
            ops.nt_x6(dh6, w1, "dx", M, dy)
        else:
            dw2, db2b = ops.linear_dw(d, a, M, D, Hd, want_bias=db2 is None, weight=w2, bias=b2)
            db2 = db2 if db2 is not None else db2b
            dh = torch.empty(M, Hd, dtype=adt, device=x.device)
            if adt == torch.bfloat16:
                # (dY W2) * gelu'(h); the epilogue also leaves per-64-row column sums of dh = fc1's bias-gradient partials
                part = torch.empty((M + 63) // 64, Hd, dtype=torch.float32, device=x.device)
                ops.linear_dx(d, M, D, w2, dh, Hd, epi=EPI_MUL8 if h.dtype == torch.uint8 else EPI_MUL, aux=h, ld_aux=Hd,
                              colsum_partial=part)                                             # h = gelu' here
                db1 = ops.colsum(part, part.shape[0], Hd, Hd, ops.grad_out(b1, (Hd,), x.device))
                dw1, _ = ops.linear_dw(dh, y, M, Hd, D, want_bias=False, weight=w1)
            else:
                ops.linear_dx(d, M, D, w2, dh, Hd, epi=EPI_DGELU, aux=h, ld_aux=Hd)
                dw1, db1 = ops.linear_dw(dh, y, M, Hd, D, weight=w1, bias=b1)
            dy = torch.empty(M, D, dtype=adt, device=x.device)
            ops.linear_dx(dh, M, Hd, w1, dy, D)
        return (*_block_ln_bwd(ctx, dy, dout, x, g, b, mean, rstd), dw1, db1, dw2, db2, None, None)


def mlp_block(x, g, b, w1, b1, w2, b2, prec, *, row_scale=None):
    """``row_scale``: as in ``attn_block``."""
    if row_scale is None:
        return _MlpBlock.apply(x, g, b, w1, b1, w2, b2, prec)
    return _MlpBlock.apply(x, g, b, w1, b1, w2, b2, prec, _row_scale_arg(x, row_scale))


# ------------------------------------------------------------------------------------------------------------
# decoders
# ------------------------------------------------------------------------------------------------------------
class _ClsHead(Function):
    """ClassificationDecoder: linear(norm(x[:, row])) with row = 0 (vit.py:335-342) -> fp32 logits [B, num_classes]."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, w, bias, prec, row=0):
        adt = ops.act_dtype(prec)
        B, T, D = x.shape
        C = w.shape[0]
        if not 0 <= row < T:
            raise ValueError(f"cls_head: row {row} is outside the sequence of {T} tokens")
        x = _c(x)
        # rows = token ``row`` of every image, T*D apart (row 0: the cls tokens)
        y, mean, rstd = ops.layernorm_fwd(x if row == 0 else x.view(-1)[row * D:], T * D, B, D, g, b, adt)
        logits = torch.empty(B, C, dtype=torch.float32, device=x.device)
        ops.linear_fwd(y, B, D, w, bias, logits, C)
        ctx.save_for_backward(x, g, mean, rstd, y, w)
        ctx.small = (b, bias)
        ctx.row = row
        return logits

    @staticmethod
    @_scoped
    def backward(ctx, dlogits):
        x, g, mean, rstd, y, w = ctx.saved_tensors
        B, T, D = x.shape
        C = w.shape[0]
        adt = y.dtype
        ld = ops.pad8(C) if adt == torch.bfloat16 else C
        dl = torch.zeros(B, ld, dtype=adt, device=x.device)
        dl[:, :C] = dlogits                                                # tiny (B x C) pad+cast: cold glue
        b, bias = ctx.small
        dw, dbias = ops.linear_dw(dl, y, B, C, D, ld_dy=ld, weight=w, bias=bias)
        dy = torch.empty(B, D, dtype=adt, device=x.device)
        ops.linear_dx(dl, B, C, w, dy, D, ld_dy=ld)
        dx = torch.zeros_like(x)
        o = ctx.row * D                                                    # the gradient goes to that row of every image
        dg, db = ops.layernorm_bwd(dy, x if o == 0 else x.view(-1)[o:], T * D, g, mean, rstd, None,
                                   dx if o == 0 else dx.view(-1)[o:], T * D, B, D, beta=b)
        return dx, dg, db, dw, dbias, None, None


def cls_head(x, g, b, w, bias, prec, row=0):
    """``row`` (an extension): the token the head reads, 0 = the cls token (the reference's decoder); the distillation head of
    ``models.distill`` reads the last one.  Only the base pointer of the LayerNorm moves: row 0 is the same launches and bits."""
    return _ClsHead.apply(x, g, b, w, bias, prec, int(row))


def _seg_small_fwd(x, g, b, w, bias, prec):
    """x[:, 1:] -> LayerNorm -> Linear(D, C): the [B*h*w, C] fp32 class map before upsampling (vit.py:359-366)."""
    adt = ops.act_dtype(prec)
    B, T, D = x.shape
    C = w.shape[0]
    npatch = T - 1
    x = _c(x)
    xp = ops.gather_patch_rows(x, B, T, D, torch.float32)                # x[:, 1:] as dense rows
    M = B * npatch
    y, mean, rstd = ops.layernorm_fwd(xp, D, M, D, g, b, adt)
    small = torch.empty(M, C, dtype=torch.float32, device=x.device)      # [B, h*w, C]
    ops.linear_fwd(y, M, D, w, bias, small, C)
    return small, (xp, g, mean, rstd, y, w), (b, bias)


def _seg_small_bwd(saved, small_params, dims, dl, ld):
    """Backward of _seg_small_fwd from d(small) given as [M, ld] in the activation dtype (columns >= C zero)."""
    xp, g, mean, rstd, y, w = saved
    b, bias = small_params
    B, T, D, C = dims
    npatch = T - 1
    M = B * npatch
    adt = y.dtype
    dw, dbias = ops.linear_dw(dl, y, M, C, D, ld_dy=ld, weight=w, bias=bias)
    dy = torch.empty(M, D, dtype=adt, device=dl.device)
    ops.linear_dx(dl, M, C, w, dy, D, ld_dy=ld)
    dx = torch.zeros(B, T, D, dtype=torch.float32, device=dl.device)
    # rows of image b start at dx[b, 1]: the patch rows of one image are contiguous, images are T*D apart
    dxp = torch.empty(M, D, dtype=torch.float32, device=dl.device)
    dg, db = ops.layernorm_bwd(dy, xp, D, g, mean, rstd, None, dxp, D, M, D, beta=b)
    dx[:, 1:, :] = dxp.view(B, npatch, D)
    return dx, dg, db, dw, dbias


class _UpsampleBilinear(Function):
    """Rearrange('b (h w) c -> b c h w') + nn.Upsample(size, 'bilinear') (vit.py:355,367-371) on a decoder output
    [B, h*w, C] consumed in place -> fp32 [B, C, S, S].  Used when the decoder runs module by module (fake-quantised
    LayerNorm / Linear); the fused heads below call the same kernels."""

    @staticmethod
    @_fwd
    def forward(ctx, small, grid, size):
        ops.require_cuda(small)
        B, hw, C = small.shape
        small = _c(small.float())
        ctx.dims = (B, C, grid, size)
        return ops.upsample_bilinear_fwd(small, hw * C, 1, C, B, C, grid, grid, size, size)

    @staticmethod
    @_scoped
    def backward(ctx, dbig):
        B, C, grid, size = ctx.dims
        dsmall = torch.empty(B, grid * grid, C, dtype=torch.float32, device=dbig.device)
        ops.upsample_bilinear_bwd(_c(dbig.float()), dsmall, grid * grid * C, 1, C, B, C, grid, grid, size, size)
        return dsmall, None, None


def upsample_bilinear(small, grid, size):
    return _UpsampleBilinear.apply(small, grid, size)


class _SegHead(Function):
    """SegmentationDecoder: upsample(rearrange(linear(norm(x[:, 1:])))) (vit.py:359-374) -> fp32 [B, C, S, S]."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, w, bias, grid, size, prec):
        B, T, D = x.shape
        C = w.shape[0]
        npatch = T - 1
        small, saved, ctx.small = _seg_small_fwd(x, g, b, w, bias, prec)
        big = ops.upsample_bilinear_fwd(small, npatch * C, 1, C, B, C, grid, grid, size, size)
        ctx.save_for_backward(*saved)
        ctx.dims = (B, T, D, C, grid, size)
        return big

    @staticmethod
    @_scoped
    def backward(ctx, dbig):
        saved = ctx.saved_tensors
        B, T, D, C, grid, size = ctx.dims
        npatch = T - 1
        M = B * npatch
        adt = saved[4].dtype
        dbig = _c(dbig.float())
        dsmall = torch.empty(M, C, dtype=torch.float32, device=dbig.device)
        ops.upsample_bilinear_bwd(dbig, dsmall, npatch * C, 1, C, B, C, grid, grid, size, size)
        ld = ops.pad8(C) if adt == torch.bfloat16 else C
        if adt == torch.bfloat16:
            dl = torch.zeros(M, ld, dtype=adt, device=dbig.device)
            dl[:, :C] = dsmall                                                # (B*196 x 17) pad+cast: cold glue
        else:
            dl = dsmall
        return (*_seg_small_bwd(saved, ctx.small, (B, T, D, C), dl, ld), None, None, None)


class _SegHeadLoss(Function):
    """SegmentationDecoder + CrossEntropyLoss() + argmax in one fused tail (mv_seg_ce_*): the [B, C, S, S] logits are
    never written (vit.py:355-374 + segmentation/train.py:188,261-265).  -> (loss, pixel accuracy, pred uint8 [B,S,S])."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, w, bias, labels, grid, size, prec):
        B, T, D = x.shape
        C = w.shape[0]
        small, saved, ctx.small = _seg_small_fwd(x, g, b, w, bias, prec)
        stats, lse, pred, labels = ops.seg_ce_fwd(small, labels, B, C, grid, grid, size, size)
        adt = ops.act_dtype(prec)
        ctx.needs = any(ctx.needs_input_grad[:5])
        if ctx.needs:
            ld = ops.pad8(C) if adt == torch.bfloat16 else C
            # the gradient of the mean loss, produced now (labels and lse are hot), scaled by the incoming g in backward
            dl = ops.seg_ce_bwd(small, labels, lse, B, C, grid, grid, size, size, grad_dtype=adt, ld=ld, stats=stats)
            ctx.save_for_backward(dl, *saved)
            ctx.dims = (B, T, D, C, ld)
        ctx.mark_non_differentiable(pred)
        return stats[0], stats[1].detach(), pred

    @staticmethod
    @_scoped
    def backward(ctx, gloss, _gacc, _gpred):
        dl, *saved = ctx.saved_tensors
        B, T, D, C, ld = ctx.dims
        dl = dl * gloss.to(dl.dtype)                                          # [B*h*w, ld]: tiny
        return (*_seg_small_bwd(saved, ctx.small, (B, T, D, C), dl, ld), None, None, None, None)


class SegLoss:
    """The training loss of the fused segmentation tail, as a validated, immutable specification (mv_seg_loss_*):

        loss = cross_entropy(z, y, weight=class_weights, label_smoothing=label_smoothing) + dice_weight * Dice

    with the soft Dice of include/myrtle_vision_hip.h over the whole batch (``dice_smooth`` in numerator and denominator).  Not a
    callable criterion: the logits it applies to are never written, so it exists on the fused tail only
    (``ViT.segmentation_loss(img, labels, loss=spec)``).  The weights are uploaded once per device, when first used there."""
    __slots__ = ("class_weights", "label_smoothing", "dice_weight", "dice_smooth", "_on")

    def __init__(self, class_weights=None, label_smoothing=0.0, dice_weight=0.0, dice_smooth=1.0):
        if class_weights is not None:
            class_weights = tuple(float(v) for v in class_weights)
            if not class_weights:
                raise ValueError("SegLoss: class_weights is empty")
            if any(not (v >= 0.0) or v == float("inf") for v in class_weights):
                raise ValueError(f"SegLoss: class_weights must be finite and >= 0, got {class_weights}")
        label_smoothing, dice_weight, dice_smooth = float(label_smoothing), float(dice_weight), float(dice_smooth)
        if not (0.0 <= label_smoothing < 1.0):
            raise ValueError(f"SegLoss: label_smoothing must lie in [0, 1), got {label_smoothing}")
        if not (dice_weight >= 0.0) or dice_weight == float("inf"):
            raise ValueError(f"SegLoss: dice_weight must be finite and >= 0, got {dice_weight}")
        if dice_weight > 0.0 and not (dice_smooth > 0.0 and dice_smooth != float("inf")):
            raise ValueError(f"SegLoss: dice_smooth must be finite and > 0 when dice_weight > 0, got {dice_smooth}")
        for k, v in (("class_weights", class_weights), ("label_smoothing", label_smoothing), ("dice_weight", dice_weight),
                     ("dice_smooth", dice_smooth), ("_on", {})):
            object.__setattr__(self, k, v)

    def __setattr__(self, name, value):
        raise AttributeError("SegLoss is immutable")

    def __repr__(self):
        return (f"SegLoss(class_weights={self.class_weights}, label_smoothing={self.label_smoothing}, "
                f"dice_weight={self.dice_weight}, dice_smooth={self.dice_smooth})")

    def check_classes(self, C):
        if self.class_weights is not None and len(self.class_weights) != C:
            raise ValueError(f"SegLoss: {len(self.class_weights)} class_weights for {C} classes")

    def weight_on(self, device):
        """fp32 [C] on ``device`` (uploaded on first use there), or None."""
        if self.class_weights is None:
            return None
        device = torch.device(device)
        t = self._on.get(device)
        if t is None:
            t = self._on[device] = torch.tensor(self.class_weights, dtype=torch.float32, device=device)
        return t


class _SegHeadLossRecipe(Function):
    """_SegHeadLoss with a SegLoss (mv_seg_loss_*) -> (loss, pixel accuracy, pred uint8 [B,S,S], areas int64 [3, C])."""

    @staticmethod
    @_fwd
    def forward(ctx, x, g, b, w, bias, labels, grid, size, spec, prec):           # prec last: _fwd reads it there
        B, T, D = x.shape
        C = w.shape[0]
        small, saved, ctx.small = _seg_small_fwd(x, g, b, w, bias, prec)
        cw = spec.weight_on(small.device)
        kw = dict(class_weight=cw, label_smoothing=spec.label_smoothing, dice_weight=spec.dice_weight)
        stats, lse, pred, coef, areas, labels = ops.seg_loss_fwd(small, labels, B, C, grid, grid, size, size,
                                                                 dice_smooth=spec.dice_smooth, **kw)
        adt = ops.act_dtype(prec)
        ctx.needs = any(ctx.needs_input_grad[:5])
        if ctx.needs:
            ld = ops.pad8(C) if adt == torch.bfloat16 else C
            # the gradient of the loss, produced now (labels and lse are hot), scaled by the incoming g in backward
            dl = ops.seg_loss_bwd(small, labels, lse, stats, coef, B, C, grid, grid, size, size, grad_dtype=adt, ld=ld, **kw)
            ctx.save_for_backward(dl, *saved)
            ctx.dims = (B, T, D, C, ld)
        ctx.mark_non_differentiable(pred, areas)
        return stats[0], stats[1].detach(), pred, areas

    @staticmethod
    @_scoped
    def backward(ctx, gloss, _gacc, _gpred, _gareas):
        dl, *saved = ctx.saved_tensors
        B, T, D, C, ld = ctx.dims
        dl = dl * gloss.to(dl.dtype)                                          # [B*h*w, ld]: tiny
        return (*_seg_small_bwd(saved, ctx.small, (B, T, D, C), dl, ld), None, None, None, None, None)


def seg_head_loss(x, g, b, w, bias, labels, grid, size, prec, loss=None):
    """``loss=None``: the plain mean cross entropy (mv_seg_ce_*) -> (loss, accuracy, pred).  A ``SegLoss``: mv_seg_loss_* ->
    (loss, accuracy, pred, areas int64 [3, C])."""
    if loss is None:
        return _SegHeadLoss.apply(x, g, b, w, bias, labels, grid, size, prec)
    if not isinstance(loss, SegLoss):
        raise TypeError(f"seg_head_loss: loss must be a SegLoss or None, got {type(loss).__name__}")
    loss.check_classes(w.shape[0])
    return _SegHeadLossRecipe.apply(x, g, b, w, bias, labels, grid, size, loss, prec)


def seg_head(x, g, b, w, bias, grid, size, prec):
    return _SegHead.apply(x, g, b, w, bias, grid, size, prec)


# ------------------------------------------------------------------------------------------------------------
# YOLOS detection: decoder, sequence assembly, set loss (csrc/detection.hip; fp32 in every precision)
# ------------------------------------------------------------------------------------------------------------
class _DetHeads(Function):
    """DetectionDecoder: class_embed(x[:, -Q:]) and bbox_embed(x[:, -Q:]).sigmoid() (vit.py:389-396) in one pass over the
    gathered rows -> fp32 (logits [B, Q, C + 1], boxes [B, Q, 4])."""

    @staticmethod
    def forward(ctx, x, w_cls, b_cls, w_box, b_box, Q):
        ops.require_cuda(x, w_cls, b_cls, w_box, b_box)
        ctx.set_materialize_grads(False)                      # an output the loss does not use arrives as None, not as zeros
        x = _c(x.float())
        logits, boxes = ops.det_heads_fwd(x, _c(w_cls.detach()), _c(b_cls.detach()), _c(w_box.detach()), _c(b_box.detach()), Q)
        ctx.save_for_backward(x, w_cls, w_box, boxes)
        ctx.params = (w_cls, b_cls, w_box, b_box)
        ctx.Q = Q
        return logits, boxes

    @staticmethod
    def backward(ctx, dlogits, dboxes):
        x, w_cls, w_box, boxes = ctx.saved_tensors
        dlogits = None if dlogits is None else _c(dlogits.float())
        dboxes = None if dboxes is None else _c(dboxes.float())
        dx, dwc, dbc, dwb, dbb = ops.det_heads_bwd(x, _c(w_cls.detach()), _c(w_box.detach()), boxes, dlogits, dboxes, ctx.Q,
                                                   want_dx=ctx.needs_input_grad[0], params=ctx.params)
        return dx, dwc, dbc, dwb, dbb, None


def det_heads(x, w_cls, b_cls, w_box, b_box, num_det_tokens):
    return _DetHeads.apply(x, w_cls, b_cls, w_box, b_box, num_det_tokens)


class _DetAppend(Function):
    """cat(x, det_tokens + pos_embedding_det) along the sequence (vit.py:285-302 with the detection branch taken)."""

    @staticmethod
    def forward(ctx, x, det_tokens, pos_det):
        ops.require_cuda(x, det_tokens, pos_det)
        Q, D = det_tokens.shape[-2:]
        ctx.dims = (x.shape[1], Q, det_tokens.shape, pos_det.shape)
        ctx.params = (det_tokens if det_tokens.is_leaf else None, pos_det if pos_det.is_leaf else None)
        return ops.det_append_fwd(_c(x.float()), ops._f32c(det_tokens).view(Q, D), ops._f32c(pos_det).view(Q, D))

    @staticmethod
    def backward(ctx, dout):
        T0, Q, det_shape, pos_shape = ctx.dims
        dx, ddet, dpos = ops.det_append_bwd(_c(dout.float()), T0, Q, *ctx.params)
        return dx, ddet.view(det_shape), dpos.view(pos_shape)


def det_append(x, det_tokens, pos_det):
    return _DetAppend.apply(x, det_tokens, pos_det)


_neg_zero_rows = {}


def _neg_zero_row(D, device):
    """fp32 [1, D] of -0.0, kept on the device: the position row that makes ``mv_det_append_*`` a plain concatenation
    (v + -0.0 is v bit for bit, for v = -0.0 and +0.0 too)."""
    key = (torch.device(device), D)
    if key not in _neg_zero_rows:
        _neg_zero_rows[key] = torch.full((1, D), -0.0, dtype=torch.float32, device=device)
    return _neg_zero_rows[key]


class _TokenAppend(Function):
    """cat(x, token) along the sequence (distill.py:65-69: the distillation token goes behind the positional add, so it has no
    position row): ``mv_det_append_*`` with Q = 1.  Backward: dx = dout[:, :T0], dtoken = the batch-ordered sum of dout[:, T0]."""

    @staticmethod
    def forward(ctx, x, token):
        ops.require_cuda(x, token)
        D = x.shape[-1]
        if token.numel() != D:
            raise ValueError(f"token_append: a token of {D} elements expected, got {tuple(token.shape)}")
        ctx.dims = (x.shape[1], token.shape)
        ctx.param = token if token.is_leaf else None
        return ops.det_append_fwd(_c(x.float()), ops._f32c(token).view(1, D), _neg_zero_row(D, x.device))

    @staticmethod
    def backward(ctx, dout):
        T0, token_shape = ctx.dims
        dx, dtoken, _ = ops.det_append_bwd(_c(dout.float()), T0, 1, ctx.param, None)
        return dx, dtoken.view(token_shape)


def token_append(x, token):
    """x fp32 [B, T0, D], token [1, 1, D] (any shape of D elements) -> [B, T0 + 1, D] with the token as the last row of every image."""
    return _TokenAppend.apply(x, token)


class _DetSetLoss(Function):
    """SetCriterion's three differentiable scalars and two statistics (detector.py:41-98) from the per-query targets:
    -> (loss_ce, loss_bbox, loss_giou, class_error, cardinality_error), one kernel each way."""

    @staticmethod
    def forward(ctx, logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes):
        ctx.set_materialize_grads(False)
        logits, boxes = _c(logits.float()), _c(boxes.float())
        stats, lse = ops.det_loss_fwd(logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes)
        ctx.save_for_backward(logits, boxes, tgt_class, tgt_box, weight, lse, stats)
        ctx.num_boxes = num_boxes
        out = stats[:5].unbind(0)
        ctx.mark_non_differentiable(out[3], out[4])
        return out

    @staticmethod
    def backward(ctx, g_ce, g_bbox, g_giou, _g3, _g4):
        logits, boxes, tgt_class, tgt_box, weight, lse, stats = ctx.saved_tensors
        g = [None if t is None else _c(t.float()) for t in (g_ce, g_bbox, g_giou)]
        dlogits, dboxes = ops.det_loss_bwd(logits, boxes, tgt_class, tgt_box, weight, lse, stats, *g, ctx.num_boxes)
        return dlogits, dboxes, None, None, None, None, None


def det_set_loss(logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes):
    return _DetSetLoss.apply(logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes)


# ------------------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------------------
class _CrossEntropy(Function):
    """nn.CrossEntropyLoss() (mean) with the gradient produced in the same pass (classification/train.py:170,250)."""

    @staticmethod
    @_fwd
    def forward(ctx, logits, labels):
        ops.require_cuda(logits, labels)
        loss, dl, _ = ops.cross_entropy(logits.float(), labels, want_grad=True)
        ctx.save_for_backward(dl)
        ctx.shape = logits.shape
        return loss.view(())

    @staticmethod
    @_scoped
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return (dl.view(ctx.shape) * g), None


def cross_entropy(logits, labels):
    return _CrossEntropy.apply(logits, labels)


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for ``torch.nn.CrossEntropyLoss()`` (mean reduction, no weights) on the HIP kernel."""

    def forward(self, logits, labels):
        return cross_entropy(logits, labels)


class _SoftCrossEntropy(Function):
    """Mean cross entropy against the Mixup / CutMix target with label smoothing (timm's ``SoftTargetCrossEntropy`` on
    ``mixup_target``'s output, neither materialised), with the gradient and the arg-max produced in the same pass."""

    @staticmethod
    @_fwd
    def forward(ctx, logits, labels, lam, smoothing, pair_flip):
        ops.require_cuda(logits, labels)
        loss, dl, am, _ = ops.cross_entropy_soft(logits.float(), labels, lam, smoothing, pair_flip, want_grad=True, want_argmax=True)
        ctx.save_for_backward(dl)
        ctx.shape, ctx.dtype = logits.shape, logits.dtype
        ctx.mark_non_differentiable(am)
        return loss.view(()), am

    @staticmethod
    @_scoped
    def backward(ctx, g, _g_argmax):
        (dl,) = ctx.saved_tensors
        return (dl.view(ctx.shape) * g).to(ctx.dtype), None, None, None, None


def soft_cross_entropy(logits, labels, lam=1.0, smoothing=0.0, pair_flip=True, return_argmax=False):
    """Mean of ``-sum_c t[i, c] * log_softmax(logits)[i, c]`` over the batch, ``t_i = lam * s(y_i) + (1 - lam) * s(y_j)`` with
    ``j = B - 1 - i`` and ``s(y)`` = ``smoothing / C`` everywhere plus ``1 - smoothing`` at ``y``.  ``lam`` is a host scalar (what
    ``utils.mixup.Mixup`` returns).  ``lam=1, smoothing=0`` is ``cross_entropy``.  ``return_argmax``: also the kernel's first-index
    arg-max of every row (int64 [B]), so an accuracy needs no further pass over the logits."""
    loss, am = _SoftCrossEntropy.apply(logits, labels, float(lam), float(smoothing), bool(pair_flip))
    return (loss, am) if return_argmax else loss


class SoftTargetCrossEntropy(torch.nn.Module):
    """The training criterion of a Mixup / CutMix / label-smoothing recipe on the HIP kernel: ``forward(logits, labels, lam)`` with
    the HARD labels of the batch and the ``lam`` its mixing drew -- timm's ``SoftTargetCrossEntropy`` without the [B, C] target.
    ``return_argmax=True`` makes ``forward`` return ``(loss, argmax)``."""

    def __init__(self, smoothing=0.0, return_argmax=False):
        super().__init__()
        if not 0.0 <= smoothing < 1.0:
            raise ValueError(f"label smoothing must lie in [0, 1), got {smoothing}")
        self.smoothing, self.return_argmax = float(smoothing), bool(return_argmax)

    def forward(self, logits, labels, lam=1.0):
        return soft_cross_entropy(logits, labels, lam, self.smoothing, True, self.return_argmax)


class _DistillLoss(Function):
    """DistillWrapper's loss (distill.py:142-151) with both gradients and the student's arg-max from one launch."""

    @staticmethod
    @_fwd
    def forward(ctx, student, distill, teacher, labels, temperature, alpha, mode, lam, smoothing, pair_flip):
        ops.require_cuda(student, distill, teacher, labels)
        loss, ds, dd, am, _ = ops.distill_loss(student.float(), distill.float(), teacher.detach().float(), labels, temperature, alpha,
                                               mode, lam, smoothing, pair_flip, want_grad=True, want_argmax=True)
        ctx.save_for_backward(ds, dd)
        ctx.dtypes = (student.dtype, distill.dtype)
        parts = loss.detach()[1:]
        ctx.mark_non_differentiable(am, parts)
        return loss[0].view(()), am, parts

    @staticmethod
    @_scoped
    def backward(ctx, g, _g_argmax, _g_parts):
        ds, dd = ctx.saved_tensors
        return ((ds * g).to(ctx.dtypes[0]), (dd * g).to(ctx.dtypes[1])) + (None,) * 8


def distill_loss(student, distill, teacher, labels, temperature=1.0, alpha=0.5, distillation_type="soft", lam=1.0, smoothing=0.0,
                 pair_flip=False, return_argmax=False, return_parts=False):
    """``alpha * CE(student, labels) + (1 - alpha) * KD(distill, teacher)`` (reference models/distill.py:142-151), KD = ``T^2 *
    kl_div(log_softmax(distill / T), softmax(teacher / T), "batchmean")`` for ``distillation_type="soft"`` (the reference) or the
    cross entropy against the teacher's arg-max for ``"hard"`` (DeiT's other variant).  The cross entropy is
    ``soft_cross_entropy``'s (``lam``, ``smoothing``, ``pair_flip``; the defaults are the plain one).  The teacher gets no gradient.
    ``return_argmax``: also the student's first-index arg-max (int64 [B]); ``return_parts``: also fp32 [2] = (CE mean, KD mean)."""
    loss, am, parts = _DistillLoss.apply(student, distill, teacher, labels, float(temperature), float(alpha), str(distillation_type),
                                         float(lam), float(smoothing), bool(pair_flip))
    out = (loss,) + ((am,) if return_argmax else ()) + ((parts,) if return_parts else ())
    return out if len(out) > 1 else loss


# ------------------------------------------------------------------------------------------------------------
# fake quantisation with straight-through gradient (utils/quantize.py:77-89)
# ------------------------------------------------------------------------------------------------------------
class _FakeQuant(Function):
    @staticmethod
    @_fwd
    def forward(ctx, x, kind, a, b):
        dtype = x.dtype
        if kind == "float":
            y = ops.quant_float(x, a, b)
        elif kind == "fixed":
            y = ops.quant_fixed(x, a, b)
        else:
            raise ValueError(kind)
        return y.to(dtype).view(x.shape)

    @staticmethod
    @_scoped
    def backward(ctx, g):
        return g, None, None, None


def fake_quant_float(x, exp_bits, man_bits):
    return _FakeQuant.apply(x, "float", exp_bits, man_bits)


def fake_quant_fixed(x, wl, fl):
    return _FakeQuant.apply(x, "fixed", wl, fl)
