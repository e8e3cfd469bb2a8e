"""Tensor-level wrappers over the C ABI (no autograd here; see ``functional.py``).

Every wrapper takes CUDA (ROCm) tensors owned by PyTorch, passes raw device pointers plus the current stream to
``libmyrtle_vision_hip.so`` and returns immediately (asynchronous).  PyTorch is used only for device memory and
streams.  CPU tensors are rejected: there is no CPU compute path in this package.

Precision: ``"bf16"`` = bf16 activations and weights on MFMA with fp32 accumulation and an fp32 residual stream
(the benchmark configuration); ``"fp32"`` = every contraction to fp32 accuracy (parity mode: bf16x6 Linear products, f32-MFMA
attention; MV_F32_GEMM=mfma puts every product on the bit-exact fmaf-chain kernels); ``"bf16x3"`` = the fp32 mode's data flow with
every nn.Linear product to 2^-16 relative instead of 2^-25 (two bf16 pieces per operand, three pairings: half the matrix-core work
of bf16x6; attention core, LayerNorm, GELU, softmax and the residual stream exactly as in ``"fp32"``) -- the cheapest arithmetic
inside BASELINE's 1e-3 end to end; ``"bf16x3h"`` = bf16x3 with the attention core on IEEE-half operands (the fused bf16 kernels
templated on the element type, fp32 sums / softmax / outputs): logits still 7x inside 1e-3 and every arg-max exact, gradients to
1.6e-3 (twelve layers of 2^-12 roundings of q and k under the exponential), 20 % faster than bf16x3.  The half core covers any
sequence up to 8 192 tokens: the whole-head kernels up to 288, the key-tiled ones above (384^2 fine-tuning, 512^2 segmentation).
The exact-fp32 attention core of ``"fp32"`` and ``"bf16x3"`` (and of the converted int8 model) does the same: the whole-head
f32-MFMA kernels up to 272 tokens, the key-tiled ones above, so no length materialises the [B, H, N, N] probabilities.
"""
import contextlib
import ctypes
import os
import threading
import weakref

import torch

from . import lib as _l
from .lib import (EPI_DGELU, EPI_EMBED, EPI_GELU, EPI_GELU_GRAD, EPI_GELU_GRAD8, EPI_MUL, EPI_MUL8, EPI_NONE, EPI_RESIDUAL,
                  EPI_SPLIT_DGELU, EPI_SPLIT_GELU, MV_BF16, MV_F32, check,
                  lib)

__all__ = ["EPI_NONE", "EPI_GELU", "EPI_RESIDUAL", "EPI_DGELU", "EPI_EMBED", "EPI_GELU_GRAD", "EPI_MUL", "EPI_GELU_GRAD8", "EPI_MUL8",
           "EPI_SPLIT_DGELU", "EPI_SPLIT_GELU"]

_DT = {torch.float32: MV_F32, torch.bfloat16: MV_BF16}
_X6_OUT = {torch.float32: MV_F32, torch.float16: _l.MV_F16}       # what the split-operand NT products (_nt_x6) can write


def act_dtype(prec: str):
    if prec == "bf16":
        return torch.bfloat16
    if prec in ("fp32", "bf16x3", "bf16x3h"):
        return torch.float32
    raise ValueError(f"unknown precision {prec!r} (expected 'bf16', 'bf16x3', 'bf16x3h' or 'fp32')")


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "myrtle_vision computes only through its HIP kernels on an MI355X: got a CPU tensor "
                "(there is no CPU fallback; move the model and inputs to 'cuda')")


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def pad8(n: int) -> int:
    return (n + 7) & ~7


class KernelTimer:
    """Optional per-launch timing of the MFMA kernels with events recorded on the launch stream (the stream handed
    to the C ABI is torch's current stream).  Used by bench.py for the live roofline figure; off by default."""

    def __init__(self, sample_every: int = 1, sample_steps=None):
        """``sample_every`` = k: only the launches of every k-th step (``next_step()``) are bracketed by events -- the
        event packets between kernels cost 1.4 ms (4 %) of a ViT-B step in which every GEMM launch is timed (rocprofv3 trace: ~300
        event records of ~5 us of idle each).  ``sample_steps``: an explicit set of step indices instead."""
        self.records = {}          # kernel name -> list of (start_event, end_event, algorithmic_flops)
        self.by_shape = {}         # shape label -> the same tuples
        self.sample_every = max(int(sample_every), 1)
        self.sample_steps = None if sample_steps is None else set(int(s) for s in sample_steps)
        self.step = -1
        self.active = True

    def next_step(self):
        self.step += 1
        self.active = (self.step in self.sample_steps) if self.sample_steps is not None else self.step % self.sample_every == 0

    def begin(self):
        if not self.active:
            return None
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def end(self, name, start, flops, shape=None):
        if start is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.records.setdefault(name, []).append((start, e, flops))
        if shape is not None:
            self.by_shape.setdefault(shape, []).append((start, e, flops))

    def shape_summary(self):
        """-> {shape label: dict(launches, avg_us, tflops)}: the same launches as ``summary`` split by product shape."""
        torch.cuda.synchronize()
        out = {}
        for shape, recs in self.by_shape.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            out[shape] = dict(launches=len(recs), avg_us=1e3 * ms / len(recs),
                              tflops=sum(f for _, _, f in recs) / (ms * 1e-3) / 1e12 if ms > 0 else 0.0)
        return out

    def summary(self):
        """-> {name: dict(launches, total_ms, avg_us, flops_per_launch, tflops)} (synchronises)."""
        torch.cuda.synchronize()
        out = {}
        for name, recs in self.records.items():
            ms = sum(s.elapsed_time(e) for s, e, _ in recs)
            fl = sum(f for _, _, f in recs)
            out[name] = dict(launches=len(recs), total_ms=ms, avg_us=1e3 * ms / len(recs), flops_per_launch=fl / len(recs),
                             tflops=fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0)
        return out


_timer = None


def set_kernel_timer(timer):
    global _timer
    _timer = timer


class _Timed:
    """One bracket of ``_timed``: the start event on entry, the record once the launches went through (none if one raised)."""
    __slots__ = ("name", "flops", "shape", "start")

    def __init__(self, name, flops, shape):
        self.name, self.flops, self.shape = name, flops, shape

    def __enter__(self):
        self.start = _timer.begin()

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            _timer.end(self.name, self.start, self.flops, shape=self.shape)


_untimed = contextlib.nullcontext()


def _timed(name, flops, shape=None):
    """``with _timed(name, flops, shape):`` around the launches of one product.  With a KernelTimer installed: one record under ``name``
    and under ``shape`` (on the steps it samples), from an event before the first launch to one after the last; else nothing at all."""
    return _untimed if _timer is None else _Timed(name, flops, shape)


_workspaces = {}


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch buffer per (device, stream): ops on one stream execute in order, so they can share it."""
    key = (device.index, _s())
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = w
    return w


# ------------------------------------------------------------------------------------------------------------
# gradient destinations
# ------------------------------------------------------------------------------------------------------------
# ``optim.ParamArena`` keeps every parameter gradient in one flat buffer (the all-reduce / AdamW operand).  The backward
# kernels write a parameter's gradient STRAIGHT into its arena slot when the parameter has no gradient yet: autograd
# then adopts the returned view as ``param.grad`` (no ``grad += new`` launch, no zero-fill of 344 MB per step).  If the
# parameter already holds a gradient (micro-batch accumulation) a fresh tensor is returned and autograd adds as usual.
_grad_slots = {}


def register_grad_slot(param, slot):
    """``slot``: flat fp32 view of ``param.numel()`` elements that must receive d(loss)/d(param)."""
    key = id(param)
    _grad_slots[key] = slot
    weakref.finalize(param, _grad_slots.pop, key, None)


def grad_slot(param):
    return _grad_slots.get(id(param)) if param is not None else None


def grad_out(param, shape, device):
    """fp32 tensor of ``shape`` for the kernels to write the gradient of ``param`` into (``param`` may be None)."""
    slot = grad_slot(param)
    if slot is not None and param.grad is None:
        n = 1
        for d in shape:
            n *= d
        if n == slot.numel():
            return slot.view(shape)
    return torch.empty(shape, dtype=torch.float32, device=device)


# ------------------------------------------------------------------------------------------------------------
# weights prepared for the MFMA path
# ------------------------------------------------------------------------------------------------------------
class PreparedWeight:
    """bf16 copies of one nn.Linear weight [N_out, K_in]: ``w`` [N_out, pad8(K_in)] for the forward product and
    ``wt`` [K_in, pad8(N_out)] (transposed) for the input-gradient product; pads are zero."""

    __slots__ = ("w", "wt", "ldw", "ldt", "n_out", "k_in", "version", "ptr", "ref", "epoch", "owner")


class _WeightPrepItem(ctypes.Structure):          # mv_weight_prep_item (include/myrtle_vision_hip.h)
    _fields_ = [("w", ctypes.c_void_p), ("w_bf16", ctypes.c_void_p), ("wt_bf16", ctypes.c_void_p), ("ldw", ctypes.c_int),
                ("ldt", ctypes.c_int), ("R", ctypes.c_int), ("C", ctypes.c_int), ("tiles_x", ctypes.c_int),
                ("first_block", ctypes.c_int)]


# Cache epoch: the prepared copies of a weight are valid while (its _version, its owner's epoch) are unchanged.  A weight's
# OWNER is the registered parameter arena whose flat buffer holds it (None for a free-standing parameter).  An owner's epoch
# moves when (a) ``invalidate_weight_caches(flat)`` names it -- ParamArena.bump_versions() after a raw-pointer write (the AdamW
# kernel), a replayed HIP graph (utils.graph) -- (b) ITS flat buffer is written through torch (its ``_version`` counts in-place
# ops on the flat tensor: loading into the arena, an EMA, a custom collective), which a parameter's own version counter never
# sees, or (c) ``invalidate_weight_caches()`` without an argument (everything).  Epochs only ever grow: an arena that dies folds
# its last version into its generation, so a value can never repeat, and one model's optimizer step does not make another
# (frozen, EMA, evaluation) model's copies stale.  One integer compare per lookup; nothing is refreshed until a weight is used.
_generation = [0]


class _Owner:
    """One registered arena: weak reference to the flat tensor, its address range, a generation counter."""
    __slots__ = ("ref", "lo", "hi", "gen", "last")

    def __init__(self, flat):
        self.ref, self.lo, self.gen, self.last = weakref.ref(flat), flat.data_ptr(), 0, flat._version
        self.hi = self.lo + flat.numel() * flat.element_size()

    def epoch(self) -> int:
        t = self.ref()
        if t is not None:
            self.last = t._version
        return self.gen + self.last


_owners = []


def register_arena(flat: torch.Tensor):
    for o in _owners:
        if o.ref() is None:
            _prep_table.pop(id(o), None)
    _owners[:] = [o for o in _owners if o.ref() is not None]
    _owners.append(_Owner(flat))


def _owner_of(weight):
    ptr = weight.data_ptr()
    for o in reversed(_owners):                     # the newest registration wins if an address range was recycled
        if o.lo <= ptr < o.hi and o.ref() is not None:
            return o
    return None


def invalidate_weight_caches(flat=None):
    """Move the epoch of the arena ``flat`` (every prepared copy of ITS parameters becomes stale), or of everything."""
    if flat is None:
        _generation[0] += 1
        return
    ptr = flat.data_ptr()
    for o in _owners:
        if o.lo == ptr and o.ref() is flat:
            o.gen += 1
            return
    _generation[0] += 1                             # not registered: be safe


def cache_epoch(owner=None) -> int:
    return _generation[0] + (owner.epoch() if owner is not None else 0)


_prepared = {}   # id(parameter) -> PreparedWeight (identity-keyed: tensors define == elementwise); entries die with the tensor
_prep_table = {}  # per owner: id(owner) -> (key (ids, pointers), uint8 item table on the device, count, total_blocks)
_capture_keep = None   # utils.graph: while a step is being captured, every device table / weight copy the capture reads is
#                        appended here, and the GraphedTrainStep keeps the list for as long as its graph exists


def _refresh_stale(device, owner, only=None):
    """After an optimizer step EVERY prepared weight of that optimizer's arena is stale: refresh them all in one launch
    (mv_weight_prep_batch) instead of one ~7 us launch per nn.Linear at its first use.  Only weights of ``owner`` are
    touched (``only``: a single weight, for free-standing parameters inside a graph capture)."""
    stale = []
    for pw in list(_prepared.values()):                      # a finalizer may pop entries while we look
        w = pw.ref() if pw.ref is not None else None
        if w is None or pw.owner is not owner or pw.w.device != device or not w.is_contiguous():
            continue
        if only is not None and w is not only:
            continue
        if pw.version != w._version or pw.ptr != w.data_ptr() or pw.epoch != cache_epoch(owner):
            stale.append((pw, w))
    if not stale:
        return
    epoch = cache_epoch(owner)
    key = tuple((id(w), w.data_ptr(), pw.w.data_ptr()) for pw, w in stale)
    ent = _prep_table.get(id(owner))
    if ent is None or ent[0] != key:
        items = (_WeightPrepItem * len(stale))()
        first = 0
        for it, (pw, w) in zip(items, stale):
            it.w, it.w_bf16, it.wt_bf16 = w.data_ptr(), pw.w.data_ptr(), pw.wt.data_ptr()
            it.ldw, it.ldt, it.R, it.C = pw.ldw, pw.ldt, pw.n_out, pw.k_in
            it.tiles_x, it.first_block = (max(pw.k_in, pw.ldw) + 63) // 64, first
            first += it.tiles_x * ((max(pw.n_out, pw.ldt) + 63) // 64)
        table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(device)
        ent = _prep_table[id(owner)] = (key, table, len(stale), first)
    _, table, count, total = ent
    if _capture_keep is not None:                            # the graph replays this launch: it owns what the launch reads
        _capture_keep.append((table, [(pw.w, pw.wt) for pw, _ in stale]))
    check(lib().mv_weight_prep_batch(_p(table), count, total, _s()), "weight_prep_batch", count=count)
    for pw, w in stale:
        pw.version, pw.ptr, pw.epoch = w._version, w.data_ptr(), epoch


def prepared_weight(weight: torch.Tensor) -> PreparedWeight:
    """Cached bf16 / transposed-bf16 copies, refreshed when the parameter changed (``_version``, storage, owner epoch)."""
    key = id(weight)
    pw = _prepared.get(key)
    if pw is not None and pw.version == weight._version and pw.ptr == weight.data_ptr() and pw.epoch == cache_epoch(pw.owner):
        return pw
    require_cuda(weight)
    n_out, k_in = weight.shape
    owner = _owner_of(weight)
    if pw is not None and pw.owner is not owner:
        pw.owner, pw.epoch = owner, -1                      # the parameter moved into (or out of) an arena
    if pw is not None and pw.n_out == n_out and pw.k_in == k_in and pw.w.device == weight.device and weight.is_contiguous():
        # this weight and every other stale one of the same arena (a free-standing weight inside a capture: itself only)
        _refresh_stale(weight.device, owner, only=weight if (owner is None and _capture_keep is not None) else None)
        if pw.version == weight._version and pw.ptr == weight.data_ptr() and pw.epoch == cache_epoch(owner):
            return pw
    if pw is None or pw.n_out != n_out or pw.k_in != k_in or pw.w.device != weight.device:
        pw = PreparedWeight()
        pw.n_out, pw.k_in, pw.owner = n_out, k_in, owner
        pw.ldw, pw.ldt = pad8(k_in), pad8(n_out)
        pw.w = torch.empty(n_out, pw.ldw, dtype=torch.bfloat16, device=weight.device)
        pw.wt = torch.empty(k_in, pw.ldt, dtype=torch.bfloat16, device=weight.device)
        pw.ref = weakref.ref(weight)
        if key not in _prepared:
            weakref.finalize(weight, _prepared.pop, key, None)
        _prepared[key] = pw
    wd = weight.detach()
    if not wd.is_contiguous():
        wd = wd.contiguous()
    if _capture_keep is not None:
        _capture_keep.append((wd, [(pw.w, pw.wt)]))
    check(lib().mv_weight_prep(_p(wd), _p(pw.w), pw.ldw, _p(pw.wt), pw.ldt, n_out, k_in, _s()), "weight_prep",
          R=n_out, C=k_in)
    pw.version, pw.ptr, pw.epoch = weight._version, weight.data_ptr(), cache_epoch(owner)
    return pw


# ------------------------------------------------------------------------------------------------------------
# LayerNorm
# ------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, ldx, rows, dim, gamma, beta, out_dtype, eps=1e-5):
    """x: fp32 tensor whose data_ptr is row 0; rows are ``ldx`` elements apart.  -> (y [rows, dim], mean, rstd)"""
    require_cuda(x, gamma, beta)
    y = torch.empty(rows, dim, dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().mv_layernorm_fwd(_p(x), ldx, _p(gamma), _p(beta), _p(y), _DT[out_dtype], _p(mean), _p(rstd), rows, dim,
                                 eps, _s()), "layernorm_fwd", rows=rows, dim=dim, ldx=ldx)
    return y, mean, rstd


def layernorm_fwd_split(x, ldx, rows, dim, gamma, beta, eps=1e-5):
    """LayerNorm whose output leaves as the bf16 pieces of the split-operand products (``split_ex(layernorm_fwd(...))`` without the
    fp32 tensor in between, bit-identical): -> (y_split [rows, nseg * dim], mean, rstd)."""
    require_cuda(x, gamma, beta)
    y = _split_buffer(rows, dim, x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    check(lib().mv_layernorm_fwd_split(_p(x), ldx, _p(gamma), _p(beta), _p(y), current_segments(), _p(mean), _p(rstd), rows, dim,
                                       eps, _s()), "layernorm_fwd_split", rows=rows, dim=dim)
    return y, mean, rstd


def layernorm_bwd(dy, x, ldx, gamma, mean, rstd, dx_add, dx, lddx, rows, dim, dx16=None, dx_colsum=None, beta=None, dx_split=None):
    """Writes dx (fp32 rows ``lddx`` apart; ``dx_add`` added if given, same layout) -> (dgamma, dbeta).
    Optional fused by-products: ``dx16`` (bf16 [rows, dim] copy of dx) or ``dx_split`` (the bf16 pieces of dx, a ``_split_buffer`` of
    the current segment count) and ``dx_colsum`` (fp32 [dim] column sums).
    ``gamma`` / ``beta`` (the parameters) select the gradient destinations (``grad_out``)."""
    require_cuda(dy, x, dx)
    dgamma = grad_out(gamma, (dim,), x.device)
    dbeta = grad_out(beta, (dim,), x.device)
    nbytes = lib().mv_layernorm_bwd_workspace_bytes(rows, dim)
    ws = workspace(nbytes, x.device)
    if dx_split is not None:
        check(lib().mv_layernorm_bwd_split(_p(dy), _DT[dy.dtype], _p(x), ldx, _p(gamma), _p(mean), _p(rstd), _p(dx_add), _p(dx),
                                           lddx, _p(dgamma), _p(dbeta), 0, _p(ws), ws.numel(), rows, dim, _p(dx_split),
                                           current_segments(), _p(dx_colsum), _s()), "layernorm_bwd_split", rows=rows, dim=dim)
        return dgamma, dbeta
    check(lib().mv_layernorm_bwd(_p(dy), _DT[dy.dtype], _p(x), ldx, _p(gamma), _p(mean), _p(rstd), _p(dx_add), _p(dx),
                                 lddx, _p(dgamma), _p(dbeta), 0, _p(ws), ws.numel(), rows, dim, _p(dx16), _p(dx_colsum), _s()),
          "layernorm_bwd", rows=rows, dim=dim)
    return dgamma, dbeta


# ------------------------------------------------------------------------------------------------------------
# fp32 Linear products on the bf16 matrix cores ("bf16x6"): each fp32 operand is split into three bf16 pieces
# (mv_split3_bf16) and ONE bf16 MFMA product contracts over the six piece pairings that matter; fp32-accurate (2^-25
# relative per product, fp32 accumulation) at ~2x the f32-MFMA kernel's rate.  mv_gemm_f32 (bit-exact k-ordered fmaf
# chain) stays the path for everything the shape rules below exclude, and for MV_F32_GEMM=mfma.
# ------------------------------------------------------------------------------------------------------------
_f32_gemm_mode = os.environ.get("MV_F32_GEMM", "bf16x6")


def set_f32_gemm(mode: str) -> str:
    """'bf16x6' (default) or 'mfma' (every fp32 product on mv_gemm_f32).  Returns the previous mode."""
    global _f32_gemm_mode
    if mode not in ("bf16x6", "mfma"):
        raise ValueError(f"f32 gemm mode {mode!r}")
    prev, _f32_gemm_mode = _f32_gemm_mode, mode
    return prev


def pad32(n: int) -> int:
    return (n + 31) & ~31


# How many SEGMENTS a split operand has: 6 = bf16x6 (three pieces per operand, six pairings: fp32-accurate, ``precision="fp32"``),
# 3 = bf16x3 (two pieces, the pairings a0 b0 + a0 b1 + a1 b0: 2^-16 relative per product, half the matrix-core work,
# ``precision="bf16x3"``).  The count is a property of the running model, carried per THREAD (forward runs on the caller's thread,
# backward on autograd's workers): ``with segments(prec_segments(prec))`` in the forward of every autograd function that holds a
# Linear product, which records it for its backward (functional._scoped).
_seg_tls = threading.local()


# ``precision="bf16x3h"`` additionally runs the attention core on IEEE-half operands (mv_attention_fwd_f16 / _bwd_f16): the scope
# value 4 = three segments + half attention (``current_segments()`` still answers 3).
def prec_segments(prec: str) -> int:
    return 4 if prec == "bf16x3h" else 3 if prec == "bf16x3" else 6


def current_segments() -> int:
    n = getattr(_seg_tls, "n", 6)
    return 3 if n == 4 else n


def half_attention() -> bool:
    return getattr(_seg_tls, "n", 6) == 4


class segments:
    def __init__(self, n: int):
        if n not in (3, 4, 6):
            raise ValueError(f"segments {n}: 3 (bf16x3), 4 (bf16x3 + half attention) or 6 (bf16x6)")
        self.n = n

    def __enter__(self):
        self.prev = getattr(_seg_tls, "n", 6)
        _seg_tls.n = self.n
        return self

    def __exit__(self, *exc):
        _seg_tls.n = self.prev
        return False


def _split_buffer(rows, cols, device):
    """[rows, nseg * cols] bf16 whose STORAGE runs on to the next multiple of 32 rows, zero-filled: the dW product walks its
    contraction (the rows) in stages of 32, and zero rows add nothing -- any token count takes the bf16x6 / bf16x3 path."""
    full = torch.empty(pad32(rows), current_segments() * cols, dtype=torch.bfloat16, device=device)
    if full.shape[0] != rows:
        full[rows:].zero_()
    return full[:rows]


def split3(x, rows, cols, ldx, role, stack=False):
    """fp32 [rows, cols] (row stride ldx) -> its bf16 segments (six, or three in a ``segments(3)`` scope): [rows, nseg * cols]
    side by side, or stacked [nseg * rows, cols] (``stack``).  role 0 = left operand of the product, 1 = right operand."""
    require_cuda(x)
    nseg = current_segments()
    if stack:
        out = torch.empty(nseg * rows, cols, dtype=torch.bfloat16, device=x.device)
        ldo, seg = cols, rows * cols
    else:
        out = _split_buffer(rows, cols, x.device)
        ldo, seg = nseg * cols, cols
    fn = lib().mv_split3_bf16 if nseg == 6 else lib().mv_split2_bf16
    check(fn(_p(x), ldx, _p(out), ldo, seg, rows, cols, role, _s()), "split3_bf16" if nseg == 6 else "split2_bf16", rows=rows,
          cols=cols)
    return out


# Activation splits shared between the dX and dW products of one backward function: inside ``split_scope()`` the last
# two role-0 side-by-side splits are kept (with a reference to their source tensor) and reused when the same tensor and
# geometry come again.  Nothing is remembered outside a scope, and a scope must not write into a tensor it has already
# split (the kernels write through raw pointers: no version counter would notice).
_split_tls = threading.local()        # backward runs on autograd's per-device worker threads: one memo per thread


class split_scope:
    def __enter__(self):
        self.prev = getattr(_split_tls, "memo", None)
        _split_tls.memo = []
        return self

    def __exit__(self, *exc):
        _split_tls.memo = self.prev
        return False


def split_act(x, rows, cols, ldx, colsum_out=None):
    """Role-0 side-by-side split [rows, 6 * cols] of an activation / gradient, memoised inside a ``split_scope``.
    ``colsum_out`` (fp32 [cols]): also leave the column sums of x there (the bias gradient when x is a dY) -- from the split
    pass itself when the split is made here, by a separate pass when it comes from the memo."""
    memo = getattr(_split_tls, "memo", None)
    make = (lambda: split3(x, rows, cols, ldx, 0)) if colsum_out is None else \
           (lambda: split_ex(x, rows, cols, ldx=ldx, colsum_out=colsum_out))
    if memo is None:
        return make()
    key = (rows, cols, ldx, x.data_ptr(), current_segments())
    for ent in memo:
        if ent[1] == key:                                    # ent[0] keeps that storage alive: the address cannot be reused
            if colsum_out is not None:
                colsum(x, rows, cols, ldx, colsum_out)
            return ent[2]
    out = make()
    memo.append((x, key, out))
    if len(memo) > 2:
        memo.pop(0)
    return out


class _SplitWeight:
    __slots__ = ("version", "ptr", "fwd", "dx", "epoch")


_split_weights = {}


def split_weight(weight: torch.Tensor, which: str) -> torch.Tensor:
    """Cached right-operand splits of an nn.Linear weight [N, K]: 'fwd' -> [N, nseg K] (y = x W^T), 'dx' -> [K, nseg N] (the
    transposed weight, dx = dy W); refreshed when the parameter changed.  One cache entry per segment count."""
    key = id(weight)
    sw = _split_weights.get(key)
    epoch = cache_epoch(_owner_of(weight))
    if sw is None or sw.version != weight._version or sw.ptr != weight.data_ptr() or sw.epoch != epoch:
        if sw is None:
            weakref.finalize(weight, _split_weights.pop, key, None)
        sw = _split_weights[key] = _SplitWeight()
        sw.version, sw.ptr, sw.fwd, sw.dx, sw.epoch = weight._version, weight.data_ptr(), {}, {}, epoch
    n_out, k_in = weight.shape
    nseg = current_segments()
    have = sw.fwd if which == "fwd" else sw.dx
    if nseg in have:
        return have[nseg]
    if weight.is_contiguous() and n_out % 2 == 0 and k_in % 2 == 0:
        # one read of w gives both layouts (mv_weight_split); a weight that takes gradients will be asked for the other one in
        # this step's backward, so both are made now -- one launch per weight and optimizer step, no transposed fp32 copy
        both = weight.requires_grad and torch.is_grad_enabled()
        want_fwd, want_dx = which == "fwd" or both, which == "dx" or both
        fwd = _split_buffer(n_out, k_in, weight.device) if want_fwd and nseg not in sw.fwd else None
        dx = _split_buffer(k_in, n_out, weight.device) if want_dx and nseg not in sw.dx else None
        check(lib().mv_weight_split(_p(weight.detach()), _p(fwd), _p(dx), n_out, k_in, nseg, _s()), "weight_split", R=n_out, C=k_in)
        if fwd is not None:
            sw.fwd[nseg] = fwd
        if dx is not None:
            sw.dx[nseg] = dx
        return have[nseg]
    if which == "fwd":
        sw.fwd[nseg] = split3(weight.detach().contiguous(), n_out, k_in, k_in, 1)
    else:
        sw.dx[nseg] = split3(weight.detach().t().contiguous(), k_in, n_out, n_out, 1)
    return have[nseg]


def _x6_nt_ok(M, N, Kc):
    """[M, N] = A[M, Kc] B[N, Kc]^T through the 8-phase kernel with a 6 * Kc contraction."""
    return _f32_gemm_mode == "bf16x6" and M >= 128 and N % 16 == 0 and N >= 64 and Kc % 64 == 0


def _x6_tn_ok(M, N, K):
    """dW[N, K] = dY[M, N]^T X[M, K] through the segmented TN ring kernel with a 6 * M contraction."""
    return _f32_gemm_mode == "bf16x6" and M >= 128 and N % 8 == 0 and K % 8 == 0


def x6_block_ok(M, *dims):
    """Whether every Linear product of a transformer block with M token rows and these feature widths takes the bf16x6
    path (forward, dX and dW): the block functions then keep the SPLITS of their activations instead of the activations."""
    return _f32_gemm_mode == "bf16x6" and M >= 128 and all(d % 64 == 0 for d in dims)


def split_ex(x, rows, cols, *, ldx=None, op=0, h=None, ldh=None, colsum_out=None):
    """Role-0 side-by-side split [rows, 6 * cols] of v = x (op 0), gelu(x) (op 1) or x * gelu'(h) (op 2); ``colsum_out``
    (fp32 [cols]) receives the column sums of v."""
    require_cuda(x)
    out = _split_buffer(rows, cols, x.device)
    ws = workspace(lib().mv_split3_ex_workspace_bytes(rows, cols), x.device) if colsum_out is not None else None
    fn = lib().mv_split3_bf16_ex if current_segments() == 6 else lib().mv_split2_bf16_ex
    check(fn(_p(x), cols if ldx is None else ldx, _p(h), cols if ldh is None else ldh, op, _p(out), rows,
                                  cols, _p(colsum_out), _p(ws), ws.numel() if ws is not None else 0, _s()),
          "split3_bf16_ex", rows=rows, cols=cols, mode=op)
    return out


def nt_x6(a6, weight, which, M, out, *, bias=None, residual=None):
    """out[M, N] = a (given as its split a6) times the Linear weight: which = 'fwd' -> a W^T (+bias) (+residual),
    'dx' -> a W.  out / residual dense fp32 [M, N]."""
    n_out, k_in = weight.shape
    N, Kc = (n_out, k_in) if which == "fwd" else (k_in, n_out)
    _nt_x6(a6, split_weight(weight, which), out, N, M, N, Kc, bias, EPI_RESIDUAL if residual is not None else EPI_NONE,
           residual, N, tag=which)
    return out


def nt_split_ok(M, N, Kc):
    """Whether the split-output epilogues of the NT kernels take [M, N] = A[M, Kc] B[N, Kc]^T (whole 256 x 256 tiles only)."""
    return M % 256 == 0 and N % 256 == 0 and (current_segments() * Kc) % 128 == 0


def nt_x6_gelu_split(y6, weight, M, h, *, bias):
    """fc1 of the split-operand modes in ONE launch: h[M, N] (fp32 pre-activation, kept for the backward) = y W^T + b and the
    bf16 pieces of gelu(h) -> [M, nseg * N] (what fc2's forward and dW products read); no split pass over h."""
    N, Kc = weight.shape
    nseg = current_segments()
    a6 = _split_buffer(M, N, h.device)
    with _timed(f"gemm_nt_bf16x{nseg}", 2.0 * M * N * Kc, f"fwd N{N} K{Kc} split-gelu"):
        check(lib().mv_gemm_nt_bf16(_p(y6), nseg * Kc, _p(split_weight(weight, "fwd")), nseg * Kc, _p(a6), nseg * N, MV_BF16, M, N,
                                    nseg * Kc, _p(bias), EPI_SPLIT_GELU, None, 0, nseg, _p(h), N, _s()),
              "gemm_nt_bf16(split gelu)", M=M, N=N, K=nseg * Kc)
    return a6


def nt_x6_dgelu_split(d6, weight, M, h, colsum_out):
    """fc2's input gradient of the split-operand modes in ONE launch: the bf16 pieces of (dY W2) * gelu'(h) -> [M, nseg * K] and its
    column sums (fc1's bias gradient) -> ``colsum_out``; no fp32 dh, no split pass."""
    N, K = weight.shape                                  # nn.Linear [out = N, in = K]: dX[M, K] = dY[M, N] W
    nseg = current_segments()
    dh6 = _split_buffer(M, K, h.device)
    part = torch.empty((M + 63) // 64, K, dtype=torch.float32, device=h.device)
    with _timed(f"gemm_nt_bf16x{nseg}", 2.0 * M * N * K, f"dx N{K} K{N} split-dgelu"):
        check(lib().mv_gemm_nt_bf16(_p(d6), nseg * N, _p(split_weight(weight, "dx")), nseg * N, _p(dh6), nseg * K, MV_BF16, M, K,
                                    nseg * N, None, EPI_SPLIT_DGELU, _p(h), K, nseg, _p(part), K, _s()),
              "gemm_nt_bf16(split dgelu)", M=M, N=K, K=nseg * N)
    colsum(part, part.shape[0], K, K, colsum_out)
    return dh6


def tn_x6(dy6, x6, M, weight):
    """dW[N, K] = dY^T X from the two splits, into the weight's gradient slot."""
    N, K = weight.shape
    dw = grad_out(weight, (N, K), dy6.device)
    _tn_segments(dy6, x6, dw, M, N, K)
    return dw


def _tn_segments(dy6, x6, dw, M, N, K):
    nseg = current_segments()
    Mp = pad32(M)                                  # the splits' storage is zero-padded to whole stages (_split_buffer)
    ws = workspace(lib().mv_gemm_tn_workspace_bytes(N, K, nseg * Mp), dy6.device)
    fn = lib().mv_gemm_tn_bf16_x6 if nseg == 6 else lib().mv_gemm_tn_bf16_x3
    with _timed(f"gemm_tn_bf16x{nseg}", 2.0 * M * N * K, f"dw N{N} K{K}"):
        check(fn(_p(dy6), _p(x6), _p(dw), K, N, K, Mp, _p(ws), ws.numel(), _s()), f"gemm_tn_bf16_x{nseg}", M=N, N=K, rows=Mp)


def _x6_ksplits(M, N):
    """K-split count of a bf16x6 NT product: 3 (two of the six segments per slice) when that shortens the schedule on
    the 256 CUs by a quarter or more -- 150 tiles: one round of 6 segments -> two rounds of 2."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    r1, r3 = -(-tiles // 256), -(-(3 * tiles) // 256) / 3.0
    return 3 if r3 <= 0.75 * r1 else 1


def _nt_x6(a6, b6, out, ldc, M, N, Kc, bias, epi, aux=None, ld_aux=0, aux_i=0, tag="fwd"):
    c_dt = _X6_OUT.get(out.dtype)
    if c_dt is None:
        raise ValueError(f"_nt_x6: the output is fp32 or IEEE half, got {out.dtype}")
    if out.dtype == torch.float16 and epi != EPI_NONE:           # half output: q / k / v of precision "bf16x3h"
        raise ValueError(f"_nt_x6: a half output takes no epilogue (EPI_NONE), got epi {epi}")
    nseg = current_segments()
    Kx = nseg * Kc
    S = _x6_ksplits(M, N) if epi in (EPI_NONE, EPI_RESIDUAL) and ldc == N and (aux is None or ld_aux == N) else 1
    if S > 1 and (Kx % (128 * S) != 0 or out.dtype != torch.float32):
        S = 1
    with _timed(f"gemm_nt_bf16x{nseg}", 2.0 * M * N * Kc, f"{tag} N{N} K{Kc} epi{epi}" + (f" S{S}" if S > 1 else "")):
        if S > 1:
            slabs = workspace(S * M * N * 4, out.device)
            check(lib().mv_gemm_nt_bf16_ksplit(_p(a6), Kx, _p(b6), Kx, _p(slabs), M, N, Kx, S, _p(bias), _s()),
                  f"gemm_nt_bf16_ksplit(x{nseg})", M=M, N=N, K=Kx, S=S)
            check(lib().mv_sum_slabs_add(_p(slabs), M * N, S, _p(aux) if epi == EPI_RESIDUAL else None, _p(out), M * N, _s()),
                  "sum_slabs_add", n=M * N)
        else:
            check(lib().mv_gemm_nt_bf16(_p(a6), Kx, _p(b6), Kx, _p(out), ldc, c_dt, M, N, Kx, _p(bias), epi, _p(aux),
                                        ld_aux, aux_i, None, 0, _s()), f"gemm_nt_bf16(x{nseg})", M=M, N=N, K=Kx, epi=epi)


# ------------------------------------------------------------------------------------------------------------
# contractions.  Logical shapes: x [M, K], W [N, K] (nn.Linear layout), y [M, N]
# ------------------------------------------------------------------------------------------------------------
def linear_fwd(x, M, K, weight, bias, out, ldc, *, lda=None, epi=EPI_NONE, aux=None, ld_aux=0, aux_i=0, out2=None,
               ld_out2=0):
    """out[M, N] (+epilogue) = x[M, K] @ weight[N, K]^T + bias.  Dispatches on x.dtype: bf16 -> the bf16 MFMA kernels;
    fp32 -> bf16x6 (fp32-accurate, on the bf16 MFMA) where the shape rules allow, else mv_gemm_f32 (f32 MFMA, fmaf-chain bits)."""
    N = weight.shape[0]
    lda = K if lda is None else lda
    if x.dtype == torch.bfloat16:
        pw = prepared_weight(weight)
        with _timed("gemm_nt_bf16", 2.0 * M * N * K, f"fwd N{N} K{K} epi{epi}"):
            check(lib().mv_gemm_nt_bf16(_p(x), lda, _p(pw.w), pw.ldw, _p(out), ldc, _DT[out.dtype], M, N, K, _p(bias), epi,
                                        _p(aux), ld_aux, aux_i, _p(out2), ld_out2, _s()),
                  "gemm_nt_bf16", M=M, N=N, K=K, epi=epi)
    elif (_x6_nt_ok(M, N, K) and out.dtype == torch.float32 and weight.dtype == torch.float32
          and (epi in (EPI_NONE, EPI_RESIDUAL, EPI_EMBED) and out2 is None
               or epi == EPI_GELU and ldc == N and (out2 is None or ld_out2 == N))):
        a6, b6 = split_act(x, M, K, lda), split_weight(weight, "fwd")
        if epi == EPI_GELU:
            # pre-activation (out2 when the caller keeps it) then the exact erf GELU as its own pass
            pre = out if out2 is None else out2
            _nt_x6(a6, b6, pre, N, M, N, K, bias, EPI_NONE)
            check(lib().mv_gelu_fwd(_p(pre), _p(out), MV_F32, M * N, _s()), "gelu_fwd", n=M * N)
        else:
            _nt_x6(a6, b6, out, ldc, M, N, K, bias, epi, aux, ld_aux, aux_i)
    else:
        w = weight.detach()
        check(lib().mv_gemm_f32(_p(x), lda, 1, 0, 0, _p(w), 1, w.stride(0), 0, 0, _p(out), ldc, 1, 0, 0, M, N, K, 1, 1,
                                1.0, 0, _p(bias), epi, _p(aux), ld_aux, aux_i, _p(out2), ld_out2, _s()),
              "gemm_f32", M=M, N=N, K=K, epi=epi)
    return out


def linear_dx(dy, M, N, weight, out, ldc, *, ld_dy=None, epi=EPI_NONE, aux=None, ld_aux=0, colsum_partial=None):
    """out[M, K] = dy[M, N] @ weight[N, K]  (optionally * gelu'(aux)).  ``colsum_partial`` (bf16 path, EPI_DGELU only):
    fp32 [ceil(M/64), K] receiving per-64-row column sums of ``out`` (bias-gradient partials)."""
    K = weight.shape[1]
    ld_dy = N if ld_dy is None else ld_dy
    if dy.dtype == torch.bfloat16:
        pw = prepared_weight(weight)
        with _timed("gemm_nt_bf16", 2.0 * M * N * K, f"dx N{K} K{N} epi{epi}"):
            check(lib().mv_gemm_nt_bf16(_p(dy), ld_dy, _p(pw.wt), pw.ldt, _p(out), ldc, _DT[out.dtype], M, K, N, None, epi,
                                        _p(aux), ld_aux, 0, _p(colsum_partial), K if colsum_partial is not None else 0, _s()),
                  "gemm_nt_bf16(dx)", M=M, N=K, K=N, epi=epi)
    elif (_x6_nt_ok(M, K, N) and out.dtype == torch.float32 and weight.dtype == torch.float32
          and (epi == EPI_NONE or epi == EPI_DGELU and ldc == K and ld_aux == K)):
        _nt_x6(split_act(dy, M, N, ld_dy), split_weight(weight, "dx"), out, ldc, M, K, N, None, EPI_NONE, tag="dx")
        if epi == EPI_DGELU:
            check(lib().mv_gelu_bwd(_p(aux), _p(out), _p(out), MV_F32, M * K, _s()), "gelu_bwd", n=M * K)
    else:
        w = weight.detach()
        check(lib().mv_gemm_f32(_p(dy), ld_dy, 1, 0, 0, _p(w), w.stride(0), 1, 0, 0, _p(out), ldc, 1, 0, 0, M, K, N, 1,
                                1, 1.0, 0, None, epi, _p(aux), ld_aux, 0, None, 0, _s()),
              "gemm_f32(dx)", M=M, N=K, K=N, epi=epi)
    return out


def linear_dw(dy, x, M, N, K, *, ld_dy=None, ldx=None, want_bias=True, weight=None, bias=None, _pair=None):
    """dW[N, K] = dy[M, N]^T @ x[M, K] (fp32), db[N] = column sums of dy.  ``weight`` / ``bias`` (the parameters, optional)
    select the gradient destinations (``grad_out``).  ``_pair`` belongs to ``linear_dw_pair`` alone."""
    if _pair is not None and type(_pair) is not _DwPair:
        raise TypeError("linear_dw: _pair is linear_dw_pair's own argument (the gradients it returns are not computed yet)")
    ld_dy = N if ld_dy is None else ld_dy
    ldx = K if ldx is None else ldx
    dw = grad_out(weight, (N, K), x.device)
    db = grad_out(bias, (N,), x.device) if want_bias else None
    if _pair is not None and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16:
        _pair.append((dy, x, M, N, K, ld_dy, ldx, dw, db))         # linear_dw_pair computes it, before it returns
    elif dy.dtype == torch.bfloat16:
        nbytes = lib().mv_gemm_tn_workspace_bytes(N, K, M)
        ws = workspace(nbytes, x.device)
        with _timed("gemm_tn_bf16(+reduce+colsum)", 2.0 * M * N * K, f"dw N{N} K{K} bias{int(want_bias)}"):
            check(lib().mv_gemm_tn_bf16(_p(dy), ld_dy, _p(x), ldx, _p(dw), K, N, K, M, 0, _p(db), _p(ws), ws.numel(), _s()),
                  "gemm_tn_bf16", M=N, N=K, Kc=M)
    elif _x6_tn_ok(M, N, K) and dy.dtype == torch.float32 and x.dtype == torch.float32:
        a6, b6 = split_act(dy, M, N, ld_dy, colsum_out=db if want_bias else None), split_act(x, M, K, ldx)
        _tn_segments(a6, b6, dw, M, N, K)
    else:
        S = f32_dw_splits(M, N, K)
        if S == 1:
            check(lib().mv_gemm_f32(_p(dy), 1, ld_dy, 0, 0, _p(x), ldx, 1, 0, 0, _p(dw), K, 1, 0, 0, N, K, M, 1, 1, 1.0, 0,
                                    None, EPI_NONE, None, 0, 0, None, 0, _s()), "gemm_f32(dw)", M=N, N=K, K=M)
        else:
            # the token dimension (50 432 rows at batch 256) split over the kernel's batch axis: S x as many workgroups for a
            # product with only 36-144 output tiles; slabs summed in a fixed order (deterministic)
            Mc = M // S
            slabs = workspace(S * N * K * 4, x.device).view(torch.float32)[:S * N * K]
            check(lib().mv_gemm_f32(_p(dy), 1, ld_dy, Mc * ld_dy, 0, _p(x), ldx, 1, Mc * ldx, 0, _p(slabs), K, 1, N * K, 0,
                                    N, K, Mc, S, 1, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, _s()),
                  "gemm_f32(dw, split)", M=N, N=K, K=Mc, S=S)
            check(lib().mv_sum_slabs(_p(slabs), N * K, S, _p(dw), N * K, 0, _s()), "sum_slabs", S=S, n=N * K)
        if want_bias:
            colsum(dy, M, N, ld_dy, db)
    return dw, db


class _TnItem(ctypes.Structure):                  # mv_tn_item (include/myrtle_vision_hip.h)
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int), ("B", ctypes.c_void_p), ("ldb", ctypes.c_int),
                ("C", ctypes.c_void_p), ("ldc", ctypes.c_int), ("M", ctypes.c_int), ("N", ctypes.c_int)]


class _DwPair(list):
    """The products ``linear_dw`` left for ``linear_dw_pair`` to compute; only ``linear_dw_pair`` makes one."""


def linear_dw_pair(M, first, second):
    """Two weight gradients over the same ``M`` token rows; each of ``first`` / ``second`` is ``(dy [M, N], x [M, K], N, K, weight,
    bias, want_bias)``.  Returns ``((dw, db), (dw, db))``, both complete, as two ``linear_dw`` calls would.  bf16 products go to
    the library as ONE group (mv_gemm_tn_bf16_group: one split-K launch and one reduce where the shapes allow it, otherwise one
    after the other as mv_gemm_tn_bf16 runs them); any other dtype is two plain ``linear_dw`` calls.  Both go through
    ``linear_dw``, the hook the dispatch tests replace."""
    waiting = _DwPair()
    outs = [linear_dw(dy, x, M, N, K, want_bias=want_bias, weight=weight, bias=bias, _pair=waiting)
            for dy, x, N, K, weight, bias, want_bias in (first, second)]
    if waiting:
        _linear_dw_group(waiting)
    return outs


def _linear_dw_group(products):
    """The bf16 products ``(dy, x, M, N, K, ld_dy, ldx, dw, db)`` -- all over the same ``M`` rows -- in one grouped split-K launch
    (mv_gemm_tn_bf16_group).  The library runs them one after another, as ``mv_gemm_tn_bf16`` would, where they cannot share one."""
    M = products[0][2]
    items = (_TnItem * len(products))()
    for it, (dy, x, m, N, K, ld_dy, ldx, dw, _db) in zip(items, products):
        assert m == M and dy.dtype == torch.bfloat16 and x.dtype == torch.bfloat16
        it.A, it.lda, it.B, it.ldb, it.C, it.ldc, it.M, it.N = _p(dy), ld_dy, _p(x), ldx, _p(dw), K, N, K
    addr = ctypes.addressof(items)
    ws = workspace(lib().mv_gemm_tn_group_workspace_bytes(addr, len(products), M), products[0][1].device)
    with _timed("gemm_tn_bf16_group(+reduce)", 2.0 * M * sum(pr[3] * pr[4] for pr in products), f"dw x{len(products)}"):
        check(lib().mv_gemm_tn_bf16_group(addr, len(products), M, _p(ws), ws.numel(), _s()), "gemm_tn_bf16_group", Kc=M,
              shapes=[(pr[3], pr[4]) for pr in products])
    for dy, _x, _m, N, _K, ld_dy, _ldx, _dw, db in products:
        if db is not None:
            colsum(dy, M, N, ld_dy, db)


def f32_dw_splits(M, N, K):
    """Number of equal token-dimension splits of the fp32 dW product [N, K] = dY[M, N]^T X[M, K]: enough for >= 2 workgroups
    per CU, each split a multiple of 16 rows and at least 512 rows long."""
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    best = 1
    for s in (2, 4, 8, 16, 32):
        if M % (16 * s) == 0 and M // s >= 512 and tiles * best < 512 and (N * K) % 4 == 0:
            best = s
    return best


def colsum(x, rows, cols, ld, out):
    ws = workspace(256 * cols * 4 + 1024, x.device)
    check(lib().mv_colsum(_p(x), _DT[x.dtype], ld, _p(out), 0, rows, cols, _p(ws), ws.numel(), _s()), "colsum",
          rows=rows, cols=cols)
    return out


# ------------------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------------------
# The length caps and widths below restate the MV_REQUIRE lines of the C entry points; tests/test_attention_path.py probes the
# built library at each cap and one past it, so the two cannot drift apart.
ATTN_SHORT_MAX_N = 320      # the whole-head kernels (mv_attention_fwd / _bwd): K and V of a head in LDS
ATTN_LONG_MAX_N = 8192      # the key-tiled kernels (mv_attention_fwd_long / _bwd_long, and their half forms _long_f16)
ATTN_F16_SHORT_MAX_N = 288  # the whole-head half kernels (mv_attention_fwd_f16 / _bwd_f16)
ATTN_F32_SHORT_MAX_N = 272  # the whole-head fp32 kernels (mv_attention_fwd_f32 / _f32_lse / _f32_q8 / _bwd_f32)
ATTN_DH_WIDTHS = (32, 128)  # head widths other than 64 with fused bf16 kernels (mv_attention_fwd_dh / _bwd_dh), any N <= 8192
# A/B switch for tools/bench_long_step.py only: False sends bf16 attention with N > 320, the half attention of bf16x3h with
# N > 288, the fp32 attention of fp32 / bf16x3 with N > 272 and bf16 attention with 32- or 128-wide heads (any N) back to the
# materialised fp32 path
ATTN_LONG = True


def attention_fused_supported(qkv_dtype, N, dim_head):
    cap = ATTN_LONG_MAX_N if ATTN_LONG else ATTN_SHORT_MAX_N
    return qkv_dtype == torch.bfloat16 and dim_head == 64 and N <= cap


def attention_dh_supported(qkv_dtype, N, dim_head):
    """The key-tiled bf16 kernels for the head widths in ``ATTN_DH_WIDTHS`` (64 has kernels of its own: ``attention_fused_supported``):
    bf16 q/k/v, N <= 8192.  They are key-tiled kernels, so ``ATTN_LONG`` off sends these widths back to the materialised path too."""
    return ATTN_LONG and qkv_dtype == torch.bfloat16 and dim_head in ATTN_DH_WIDTHS and N <= ATTN_LONG_MAX_N


def attention_f32_fused_supported(qkv_dtype, N, dim_head):
    """The exact-fp32 attention core (precisions "fp32" and "bf16x3", the converted int8 model): fp32 q/k/v, N <= 8192 (the
    whole-head kernels up to 272 tokens, the key-tiled ones above; 272 with ``ATTN_LONG`` off)."""
    cap = ATTN_LONG_MAX_N if ATTN_LONG else ATTN_F32_SHORT_MAX_N
    return qkv_dtype == torch.float32 and dim_head == 64 and N <= cap


def attention_f16_supported(qkv_dtype, N, dim_head):
    """The half-operand attention core of precision "bf16x3h" (the bf16 kernels instantiated on IEEE half): fp32 q/k/v, N <= 8192
    (the whole-head kernels up to 288 tokens, the key-tiled ones above; 288 with ``ATTN_LONG`` off)."""
    cap = ATTN_LONG_MAX_N if ATTN_LONG else ATTN_F16_SHORT_MAX_N
    return qkv_dtype == torch.float32 and dim_head == 64 and N <= cap and half_attention()


# One name per forward / backward pair of wrappers.  ``attention_path`` is the only place a family is chosen; the forward
# records the name and ``attention_backward`` takes it back, so the two cannot disagree.
ATTN_BF16 = "bf16"            # attention_fwd / attention_bwd: bf16 q/k/v, 64-wide heads
ATTN_BF16_DH = "bf16_dh"      # attention_fwd_dh / attention_bwd_dh: bf16 q/k/v, the widths of ATTN_DH_WIDTHS
ATTN_F16 = "f16"              # attention_fwd_f16 / attention_bwd_f16: half q/k/v, fp32 out (precision "bf16x3h")
ATTN_F32 = "f32"              # attention_fwd_f32_lse / attention_bwd_f32_fused: exact fp32, keeps the log-sum-exp
ATTN_F32_EVAL = "f32_eval"    # attention_fwd_f32: exact fp32, nothing kept, no backward
ATTN_PROBS = "probs"          # attention_probs_fp32 + attention_pv_fp32 / attention_bwd_fp32: fp32 [B, H, N, N] probabilities
ATTN_COLSUM_PATHS = (ATTN_BF16, ATTN_BF16_DH, ATTN_F16)     # whose backward kernels fill ``colsum`` themselves


def attention_path(qkv_dtype, N, dim_head, *, need_grad, half_ok=False, hook=False):
    """Which family computes the attention core of q/k/v in ``qkv_dtype`` (for ``ATTN_F16``: the dtype they have before the half
    rounding, fp32).  ``need_grad`` only tells the two exact-fp32 paths apart; ``half_ok``: the caller can produce half q/k/v
    (the split-operand block inside a "bf16x3h" scope); ``hook``: somebody wants to see the probabilities."""
    if hook:
        return ATTN_PROBS
    if attention_fused_supported(qkv_dtype, N, dim_head):
        return ATTN_BF16
    if attention_dh_supported(qkv_dtype, N, dim_head):
        return ATTN_BF16_DH
    if half_ok and attention_f16_supported(qkv_dtype, N, dim_head):
        return ATTN_F16
    if attention_f32_fused_supported(qkv_dtype, N, dim_head):
        return ATTN_F32 if need_grad else ATTN_F32_EVAL
    return ATTN_PROBS


def attention_forward(path, qkv, B, N, H, dim_head, scale):
    """-> (out, saved) on ``path``: saved = the log-sum-exp (the fused paths), the probabilities (``ATTN_PROBS``, which takes fp32
    q/k/v and gives fp32 out: the casts are the caller's) or None (``ATTN_F32_EVAL``)."""
    if path == ATTN_BF16:
        return attention_fwd(qkv, B, N, H, scale)
    if path == ATTN_BF16_DH:
        return attention_fwd_dh(qkv, B, N, H, dim_head, scale)
    if path == ATTN_F16:
        return attention_fwd_f16(qkv, B, N, H, scale)
    if path == ATTN_F32:
        return attention_fwd_f32_lse(qkv, B, N, H, scale)
    if path == ATTN_F32_EVAL:
        return attention_fwd_f32(qkv, B, N, H, scale), None
    if path == ATTN_PROBS:
        probs = attention_probs_fp32(qkv, B, N, H, dim_head, scale)
        return attention_pv_fp32(probs, qkv, B, N, H, dim_head), probs
    raise ValueError(f"attention_forward: unknown path {path!r}")


def attention_backward(path, qkv, out, dout, saved, B, N, H, dim_head, scale, *, split=False, colsum=None):
    """-> dqkv from what ``attention_forward(path, ...)`` took and returned (``out`` is not read on ``ATTN_PROBS``).  ``colsum``
    (fp32 [B, 3*H*dim_head]: per-image column sums of dqkv) is filled by the paths of ``ATTN_COLSUM_PATHS`` only and ``split``
    (dqkv as its bf16 pieces) exists on ``ATTN_F16`` only: elsewhere the caller takes both from a pass over dqkv."""
    assert colsum is None or path in ATTN_COLSUM_PATHS, f"attention path {path!r} does not fill colsum"
    assert not split or path == ATTN_F16, f"attention path {path!r} does not write split dqkv"
    if path == ATTN_BF16:
        return attention_bwd(qkv, out, dout, saved, B, N, H, scale, colsum=colsum)
    if path == ATTN_BF16_DH:
        return attention_bwd_dh(qkv, out, dout, saved, B, N, H, dim_head, scale, colsum=colsum)
    if path == ATTN_F16:
        return attention_bwd_f16(qkv, out, dout, saved, B, N, H, scale, split=split, colsum=colsum)
    if path == ATTN_F32:
        return attention_bwd_f32_fused(qkv, out, dout, saved, B, N, H, scale)
    if path == ATTN_PROBS:
        return attention_bwd_fp32(saved, qkv, dout, B, N, H, dim_head, scale)
    raise ValueError(f"attention_backward: path {path!r} has no backward")


# Workspaces and results are torch allocations throughout (graph capture).
def _attn_rows(like, B, N, H):
    """fp32 [B, H, N]: one value per query row -- a log-sum-exp, or the delta workspace of a key-tiled backward."""
    return torch.empty(B, H, N, dtype=torch.float32, device=like.device)


def _attn_out(qkv, B, N, H, dtype, dim_head=64):
    """(out [B, N, H*dim_head] in ``dtype``, lse fp32 [B, H, N])."""
    return torch.empty(B, N, H * dim_head, dtype=dtype, device=qkv.device), _attn_rows(qkv, B, N, H)


def attention_fwd(qkv, B, N, H, scale):
    """qkv bf16 [B, N, 3*H*64] -> (out bf16 [B, N, H*64], lse fp32 [B, H, N]); N > 320 takes the key-tiled kernel."""
    if N > ATTN_SHORT_MAX_N:
        return attention_fwd_long(qkv, B, N, H, scale)
    require_cuda(qkv)
    out, lse = _attn_out(qkv, B, N, H, torch.bfloat16)
    check(lib().mv_attention_fwd(_p(qkv), _p(out), _p(lse), B, N, H, scale, _s()), "attention_fwd", B=B, N=N, H=H)
    return out, lse


def attention_bwd(qkv, out, dout, lse, B, N, H, scale, colsum=None):
    """-> dqkv.  ``colsum`` (optional fp32 [B, 3*H*64]) receives per-image column sums of dqkv (bias-gradient partials).
    N > 320 takes the key-tiled kernels."""
    if N > ATTN_SHORT_MAX_N:
        return attention_bwd_long(qkv, out, dout, lse, B, N, H, scale, colsum=colsum)
    dqkv = torch.empty_like(qkv)
    check(lib().mv_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _p(colsum), B, N, H, scale, _s()),
          "attention_bwd", B=B, N=N, H=H)
    return dqkv


def attention_fwd_long(qkv, B, N, H, scale):
    """The key-tiled forward (any N <= 8192): as ``attention_fwd``."""
    require_cuda(qkv)
    out, lse = _attn_out(qkv, B, N, H, torch.bfloat16)
    check(lib().mv_attention_fwd_long(_p(qkv), _p(out), _p(lse), B, N, H, scale, _s()), "attention_fwd_long", B=B, N=N, H=H)
    return out, lse


def attention_bwd_long(qkv, out, dout, lse, B, N, H, scale, colsum=None):
    """The key-tiled backward (any N <= 8192): as ``attention_bwd``; the delta workspace is a torch allocation (graph capture)."""
    require_cuda(qkv, out, dout, lse)
    dqkv, delta = torch.empty_like(qkv), _attn_rows(qkv, B, N, H)
    check(lib().mv_attention_bwd_long(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), _p(colsum), B, N, H, scale,
                                      _s()), "attention_bwd_long", B=B, N=N, H=H)
    return dqkv


def attention_fwd_dh(qkv, B, N, H, dim_head, scale):
    """qkv bf16 [B, N, 3*H*dim_head] -> (out bf16 [B, N, H*dim_head], lse fp32 [B, H, N]); dim_head 32 or 128, any N <= 8192."""
    require_cuda(qkv)
    out, lse = _attn_out(qkv, B, N, H, torch.bfloat16, dim_head)
    check(lib().mv_attention_fwd_dh(_p(qkv), _p(out), _p(lse), B, N, H, dim_head, scale, _s()), "attention_fwd_dh", B=B, N=N, H=H,
          dim_head=dim_head)
    return out, lse


def attention_bwd_dh(qkv, out, dout, lse, B, N, H, dim_head, scale, colsum=None):
    """-> dqkv, as ``attention_bwd_long`` for dim_head 32 or 128 (``colsum``: optional fp32 [B, 3*H*dim_head]); the delta workspace
    is a torch allocation (graph capture)."""
    require_cuda(qkv, out, dout, lse)
    dqkv, delta = torch.empty_like(qkv), _attn_rows(qkv, B, N, H)
    check(lib().mv_attention_bwd_dh(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), _p(colsum), B, N, H, dim_head, scale,
                                    _s()), "attention_bwd_dh", B=B, N=N, H=H, dim_head=dim_head)
    return dqkv


def cast_f16(src):
    """fp32 -> IEEE half (stored in a torch.float16 tensor)."""
    require_cuda(src)
    out = torch.empty(src.shape, dtype=torch.float16, device=src.device)
    check(lib().mv_cast(_p(src), MV_F32, _p(out), _l.MV_F16, src.numel(), _s()), "cast(f16)", n=src.numel())
    return out


def attention_fwd_f16(qkv16, B, N, H, scale):
    """-> (out fp32 [B, N, H*64], lse fp32 [B, H, N]) from half q/k/v [B, N, 3, H, 64]; N > 288 takes the key-tiled kernel."""
    if N > ATTN_F16_SHORT_MAX_N:
        return attention_fwd_long_f16(qkv16, B, N, H, scale)
    out, lse = _attn_out(qkv16, B, N, H, torch.float32)
    check(lib().mv_attention_fwd_f16(_p(qkv16), _p(out), _p(lse), B, N, H, scale, _s()), "attention_fwd_f16", B=B, N=N, H=H)
    return out, lse


def _attention_bwd_prep_f16(out, dout, B, N, H):
    """dout fp32 -> (dout16 half scaled per (image, head) by gscale, delta = rowsum(dout16 * out), gscale fp32 [B * H])."""
    dout16 = torch.empty(B, N, H * 64, dtype=torch.float16, device=out.device)
    delta = _attn_rows(out, B, N, H)
    gscale = torch.empty(B * H, dtype=torch.float32, device=out.device)
    check(lib().mv_attention_bwd_prep_f16(_p(dout), _p(out), _p(dout16), _p(delta), _p(gscale), B, N, H, _s()),
          "attention_bwd_prep_f16", B=B, N=N, H=H)
    return dout16, delta, gscale


def _attention_bwd_start_f16(out, dout, B, N, H, split):
    """What both half backwards start from: the prep pass, then -> (dout16, delta, gscale, dqkv, nseg) with dqkv the fp32 result
    buffer [B, N, 3*H*64] (nseg 0) or, with ``split``, the buffer of its bf16 pieces [B * N, nseg * 3*H*64]."""
    prep = _attention_bwd_prep_f16(out, dout, B, N, H)
    if split:
        return (*prep, _split_buffer(B * N, 3 * H * 64, out.device), current_segments())
    return (*prep, torch.empty(B, N, 3 * H * 64, dtype=torch.float32, device=out.device), 0)


def attention_bwd_f16(qkv16, out, dout, lse, B, N, H, scale, split=False, colsum=None):
    """-> dqkv [B, N, 3*H*64]: fp32, or (``split``) its bf16 pieces [B * N, nseg * 3*H*64] for the to_qkv dW / dX products.  ``out``
    / ``dout`` fp32 [B, N, H*64]: dout is scaled into half's range per (image, head) by a power of two taken from its own largest
    magnitude (one pass that also leaves delta); the kernel divides the factor out of its outputs.  ``colsum``: fp32 [B, 3*H*64]
    receiving per-image column sums of dqkv (to_qkv's bias gradient after a sum over images).  N > 288 takes the key-tiled
    kernels."""
    if N > ATTN_F16_SHORT_MAX_N:
        return attention_bwd_long_f16(qkv16, out, dout, lse, B, N, H, scale, split=split, colsum=colsum)
    dout16, delta, gscale, dqkv, nseg = _attention_bwd_start_f16(out, dout, B, N, H, split)
    check(lib().mv_attention_bwd_f16(_p(qkv16), _p(dout16), _p(delta), _p(lse), _p(gscale), _p(dqkv), nseg, _p(colsum), B, N, H,
                                     scale, _s()), "attention_bwd_f16", B=B, N=N, H=H)
    return dqkv


def attention_fwd_long_f16(qkv16, B, N, H, scale):
    """The key-tiled half forward (any N <= 8192): as ``attention_fwd_f16``."""
    require_cuda(qkv16)
    out, lse = _attn_out(qkv16, B, N, H, torch.float32)
    check(lib().mv_attention_fwd_long_f16(_p(qkv16), _p(out), _p(lse), B, N, H, scale, _s()), "attention_fwd_long_f16",
          B=B, N=N, H=H)
    return out, lse


def attention_bwd_long_f16(qkv16, out, dout, lse, B, N, H, scale, split=False, colsum=None):
    """The key-tiled half backward (any N <= 8192): as ``attention_bwd_f16``.  With ``colsum`` the per-block column-sum workspace
    [B, ceil(N / 128), 3*H*64] is a torch allocation, like the prep outputs (graph capture)."""
    require_cuda(qkv16, out, dout, lse)
    dout16, delta, gscale, dqkv, nseg = _attention_bwd_start_f16(out, dout, B, N, H, split)
    ws = torch.empty(B, (N + 127) // 128, 3 * H * 64, dtype=torch.float32, device=qkv16.device) if colsum is not None else None
    check(lib().mv_attention_bwd_long_f16(_p(qkv16), _p(dout16), _p(delta), _p(lse), _p(gscale), _p(dqkv), nseg, _p(colsum),
                                          _p(ws), B, N, H, scale, _s()), "attention_bwd_long_f16", B=B, N=N, H=H)
    return dqkv


def attention_fwd_f32(qkv, B, N, H, scale):
    """Exact fp32 attention core, forward only (no probabilities kept): qkv fp32 [B, N, 3*H*64] -> out fp32 [B, N, H*64].
    N > 272 takes the key-tiled kernel."""
    if N > ATTN_F32_SHORT_MAX_N:
        return attention_fwd_long_f32(qkv, B, N, H, scale, lse=False)
    require_cuda(qkv)
    out = torch.empty(B, N, H * 64, dtype=torch.float32, device=qkv.device)
    check(lib().mv_attention_fwd_f32(_p(qkv), _p(out), B, N, H, scale, _s()), "attention_fwd_f32", B=B, N=N, H=H)
    return out


def attention_fwd_f32_lse(qkv, B, N, H, scale):
    """fp32 attention core for training: -> (out fp32 [B, N, H*64], lse fp32 [B, H, N]); no probabilities are kept.
    N > 272 takes the key-tiled kernel."""
    if N > ATTN_F32_SHORT_MAX_N:
        return attention_fwd_long_f32(qkv, B, N, H, scale)
    require_cuda(qkv)
    out, lse = _attn_out(qkv, B, N, H, torch.float32)
    check(lib().mv_attention_fwd_f32_lse(_p(qkv), _p(out), _p(lse), B, N, H, scale, _s()), "attention_fwd_f32_lse",
          B=B, N=N, H=H)
    return out, lse


def attention_bwd_f32_fused(qkv, out, dout, lse, B, N, H, scale):
    """-> dqkv fp32 (qkv's layout) from the saved output and log-sum-exp.  N > 272 takes the key-tiled kernels."""
    if N > ATTN_F32_SHORT_MAX_N:
        return attention_bwd_long_f32(qkv, out, dout, lse, B, N, H, scale)
    dqkv = torch.empty_like(qkv)
    check(lib().mv_attention_bwd_f32(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), B, N, H, scale, _s()),
          "attention_bwd_f32", B=B, N=N, H=H)
    return dqkv


def attention_fwd_long_f32(qkv, B, N, H, scale, lse=True):
    """The key-tiled exact-fp32 forward (any N <= 8192): -> (out, lse) as ``attention_fwd_f32_lse``, or out alone (``lse=False``,
    as ``attention_fwd_f32``)."""
    require_cuda(qkv)
    out = torch.empty(B, N, H * 64, dtype=torch.float32, device=qkv.device)
    lse_t = _attn_rows(qkv, B, N, H) if lse else None
    check(lib().mv_attention_fwd_long_f32(_p(qkv), _p(out), _p(lse_t), B, N, H, scale, _s()), "attention_fwd_long_f32",
          B=B, N=N, H=H)
    return (out, lse_t) if lse else out


def attention_bwd_long_f32(qkv, out, dout, lse, B, N, H, scale):
    """The key-tiled exact-fp32 backward (any N <= 8192): as ``attention_bwd_f32_fused``; the delta workspace is a torch
    allocation (graph capture)."""
    require_cuda(qkv, out, dout, lse)
    dqkv, delta = torch.empty_like(qkv), _attn_rows(qkv, B, N, H)
    check(lib().mv_attention_bwd_long_f32(_p(qkv), _p(out), _p(dout), _p(lse), _p(delta), _p(dqkv), B, N, H, scale, _s()),
          "attention_bwd_long_f32", B=B, N=N, H=H)
    return dqkv


def attention_fwd_f32_q8(qkv, B, N, H, scale, q_scale, q_zero_point):
    """Exact fp32 attention core whose output goes straight into a quint8 quantiser: -> int8 codes [B, N, H*64].  N > 272 takes
    the key-tiled kernel."""
    if N > ATTN_F32_SHORT_MAX_N:
        return attention_fwd_long_f32_q8(qkv, B, N, H, scale, q_scale, q_zero_point)
    require_cuda(qkv)
    codes = torch.empty(B, N, H * 64, dtype=torch.int8, device=qkv.device)
    check(lib().mv_attention_fwd_f32_q8(_p(qkv), _p(codes), B, N, H, scale, float(q_scale), int(q_zero_point), _s()),
          "attention_fwd_f32_q8", B=B, N=N, H=H)
    return codes


def attention_fwd_long_f32_q8(qkv, B, N, H, scale, q_scale, q_zero_point):
    """The key-tiled form of ``attention_fwd_f32_q8`` (any N <= 8192)."""
    require_cuda(qkv)
    codes = torch.empty(B, N, H * 64, dtype=torch.int8, device=qkv.device)
    check(lib().mv_attention_fwd_long_f32_q8(_p(qkv), _p(codes), B, N, H, scale, float(q_scale), int(q_zero_point), _s()),
          "attention_fwd_long_f32_q8", B=B, N=N, H=H)
    return codes


def attention_probs_fp32(qkv, B, N, H, dh, scale):
    """Materialised path (fp32): probs[B, H, N, N] = softmax(q k^T * scale).  qkv fp32 [B, N, 3, H, dh]."""
    D = H * dh
    scores = torch.empty(B, H, N, N, dtype=torch.float32, device=qkv.device)
    # A = q: [m=n, k=d] strides (3D, 1), batches b: N*3D, h: dh.  B[k=d][n=j] = k[j][d]: strides (1, 3D), offset D
    k_view = qkv.view(-1)[D:]
    check(lib().mv_gemm_f32(_p(qkv), 3 * D, 1, N * 3 * D, dh, _p(k_view), 1, 3 * D, N * 3 * D, dh, _p(scores), N, 1,
                            H * N * N, N * N, N, N, dh, B, H, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, _s()),
          "gemm_f32(qk^T)", B=B, H=H, N=N)
    probs = torch.empty_like(scores)
    check(lib().mv_softmax_fwd(_p(scores), _p(probs), B * H * N, N, scale, _s()), "softmax_fwd", rows=B * H * N, cols=N)
    return probs


def attention_pv_fp32(probs, qkv, B, N, H, dh):
    D = H * dh
    out = torch.empty(B, N, D, dtype=torch.float32, device=qkv.device)
    v_view = qkv.view(-1)[2 * D:]
    check(lib().mv_gemm_f32(_p(probs), N, 1, H * N * N, N * N, _p(v_view), 3 * D, 1, N * 3 * D, dh, _p(out), D, 1,
                            N * D, dh, N, dh, N, B, H, 1.0, 0, None, EPI_NONE, None, 0, 0, None, 0, _s()),
          "gemm_f32(pv)", B=B, H=H, N=N)
    return out


def attention_bwd_fp32(probs, qkv, dout, B, N, H, dh, scale):
    """-> dqkv fp32 [B, N, 3, H, dh]"""
    D = H * dh
    dev = qkv.device
    L = lib()
    dqkv = torch.empty_like(qkv)
    flat, dflat = qkv.view(-1), dqkv.view(-1)
    k_view, v_view = flat[D:], flat[2 * D:]
    dk_view, dv_view = dflat[D:], dflat[2 * D:]
    bq, hq = N * 3 * D, dh            # batch strides inside qkv-shaped tensors
    bp, hp = H * N * N, N * N         # batch strides inside [B,H,N,N]
    bo, ho = N * D, dh                # batch strides inside [B,N,D]
    # dP[n][j] = sum_d dO[n][d] V[j][d]
    dP = torch.empty(B, H, N, N, dtype=torch.float32, device=dev)
    check(L.mv_gemm_f32(_p(dout), D, 1, bo, ho, _p(v_view), 1, 3 * D, bq, hq, _p(dP), N, 1, bp, hp, N, N, dh, B, H, 1.0, 0,
                        None, EPI_NONE, None, 0, 0, None, 0, _s()), "gemm_f32(dP)")
    # dV[j][d] = sum_n P[n][j] dO[n][d]
    check(L.mv_gemm_f32(_p(probs), 1, N, bp, hp, _p(dout), D, 1, bo, ho, _p(dv_view), 3 * D, 1, bq, hq, N, dh, N, B, H, 1.0,
                        0, None, EPI_NONE, None, 0, 0, None, 0, _s()), "gemm_f32(dV)")
    dS = torch.empty_like(dP)
    check(L.mv_softmax_bwd(_p(probs), _p(dP), _p(dS), B * H * N, N, scale, _s()), "softmax_bwd")
    # dQ[n][d] = sum_j dS[n][j] K[j][d]
    check(L.mv_gemm_f32(_p(dS), N, 1, bp, hp, _p(k_view), 3 * D, 1, bq, hq, _p(dqkv), 3 * D, 1, bq, hq, N, dh, N, B, H, 1.0,
                        0, None, EPI_NONE, None, 0, 0, None, 0, _s()), "gemm_f32(dQ)")
    # dK[j][d] = sum_n dS[n][j] Q[n][d]
    check(L.mv_gemm_f32(_p(dS), 1, N, bp, hp, _p(qkv), 3 * D, 1, bq, hq, _p(dk_view), 3 * D, 1, bq, hq, N, dh, N, B, H, 1.0,
                        0, None, EPI_NONE, None, 0, 0, None, 0, _s()), "gemm_f32(dK)")
    return dqkv


# ------------------------------------------------------------------------------------------------------------
# embedding assembly, casts, elementwise
# ------------------------------------------------------------------------------------------------------------
def patchify(img, p, out_dtype):
    require_cuda(img)
    B, C, H, W = img.shape
    if img.dtype != torch.float32 or not img.is_contiguous():
        img = img.float().contiguous()
    out = torch.empty(B * (H // p) * (W // p), p * p * C, dtype=out_dtype, device=img.device)
    check(lib().mv_patchify(_p(img), _p(out), _DT[out_dtype], B, C, H, W, p, _s()), "patchify", B=B, C=C, H=H, W=W, p=p)
    return out


def embed_cls(cls, pos, x, B, T, D):
    check(lib().mv_embed_cls(_p(cls), _p(pos), _p(x), B, T, D, _s()), "embed_cls", B=B, T=T, D=D)


def embed_bwd(dx, B, T, D, pos=None, cls_token=None):
    dpos = grad_out(pos, (T, D), dx.device)
    dcls = grad_out(cls_token, (D,), dx.device)
    check(lib().mv_embed_bwd(_p(dx), _p(dpos), _p(dcls), 0, B, T, D, _s()), "embed_bwd", B=B, T=T, D=D)
    return dpos, dcls


def embed_bwd_gather(dx, B, T, D, out_dtype, pos=None, cls_token=None):
    """One pass over dx [B, T, D]: (dpos [T, D], dcls [D], dy [B * (T - 1), D] in ``out_dtype``)."""
    dpos = grad_out(pos, (T, D), dx.device)
    dcls = grad_out(cls_token, (D,), dx.device)
    dy = torch.empty(B * (T - 1), D, dtype=out_dtype, device=dx.device)
    check(lib().mv_embed_bwd_gather(_p(dx), _p(dy), _DT[out_dtype], _p(dpos), _p(dcls), B, T, D, _s()), "embed_bwd_gather",
          B=B, T=T, D=D)
    return dpos, dcls, dy


POS_RESIZE_MAX_SIDE = 1024    # per side of the source and the target grid (mv_pos_resize_fwd / _bwd)


def pos_resize_supported(D, gh, gw, sh=14, sw=14):
    """Restates the MV_REQUIRE lines of mv_pos_resize_fwd / _bwd: D % 4 == 0, every side in 1 .. 1024."""
    return D > 0 and D % 4 == 0 and all(0 < s <= POS_RESIZE_MAX_SIDE for s in (gh, gw, sh, sw))


def pos_resize_fwd(pos, gh, gw, sh=14, sw=14, out=None):
    """pos fp32 [1 + sh*sw, D] -> [1 + gh*gw, D]: the cls row as is, the (sh, sw) grid bicubically resized to (gh, gw) (vit.py:292-302)."""
    require_cuda(pos)
    D = pos.shape[-1]
    if out is None:
        out = torch.empty(1 + gh * gw, D, dtype=torch.float32, device=pos.device)
    check(lib().mv_pos_resize_fwd(_p(pos), _p(out), sh, sw, gh, gw, D, _s()), "pos_resize_fwd", sh=sh, sw=sw, gh=gh, gw=gw, D=D)
    return out


def pos_resize_bwd(dout, gh, gw, param=None, sh=14, sw=14, out=None, accumulate=False):
    """dout fp32 [1 + gh*gw, D] -> dpos [1 + sh*sw, D], the transpose of ``pos_resize_fwd``.  ``param`` (the parameter) selects the
    gradient destination (``grad_out``); ``out`` names one explicitly, ``accumulate`` adds into it instead of overwriting."""
    require_cuda(dout)
    D = dout.shape[-1]
    dpos = out if out is not None else grad_out(param, (1 + sh * sw, D), dout.device)
    check(lib().mv_pos_resize_bwd(_p(dout), _p(dpos), int(bool(accumulate)), sh, sw, gh, gw, D, _s()), "pos_resize_bwd", sh=sh,
          sw=sw, gh=gh, gw=gw, D=D)
    return dpos


def gather_patch_rows(src, B, T, D, out_dtype):
    out = torch.empty(B * (T - 1), D, dtype=out_dtype, device=src.device)
    check(lib().mv_gather_patch_rows(_p(src), _p(out), _DT[out_dtype], B, T, D, _s()), "gather_patch_rows", B=B, T=T, D=D)
    return out


def cast(src, out_dtype):
    require_cuda(src)
    if src.dtype == out_dtype:
        return src
    out = torch.empty(src.shape, dtype=out_dtype, device=src.device)
    check(lib().mv_cast(_p(src), _DT[src.dtype], _p(out), _DT[out_dtype], src.numel(), _s()), "cast", n=src.numel())
    return out


def cast_into(src, dst):
    """dst <- src with a dtype conversion, into caller-owned storage (the DDP exchange's bf16 staging copies)."""
    require_cuda(src, dst)
    if src.numel() != dst.numel() or not (src.is_contiguous() and dst.is_contiguous()):
        raise ValueError("cast_into: contiguous tensors of equal size")
    check(lib().mv_cast(_p(src), _DT[src.dtype], _p(dst), _DT[dst.dtype], src.numel(), _s()), "cast", n=src.numel())
    return dst


def gelu_fwd(x):
    y = torch.empty_like(x)
    check(lib().mv_gelu_fwd(_p(x), _p(y), _DT[x.dtype], x.numel(), _s()), "gelu_fwd", n=x.numel())
    return y


def gelu_bwd(x, dy):
    dx = torch.empty_like(x)
    check(lib().mv_gelu_bwd(_p(x), _p(dy), _p(dx), _DT[x.dtype], x.numel(), _s()), "gelu_bwd", n=x.numel())
    return dx


def add_f32(a, b):
    out = torch.empty_like(a)
    check(lib().mv_add_f32(_p(a), _p(b), _p(out), a.numel(), _s()), "add_f32", n=a.numel())
    return out


# ------------------------------------------------------------------------------------------------------------
# fake quantisation
# ------------------------------------------------------------------------------------------------------------
def quant_float(x, exp_bits, man_bits):
    require_cuda(x)
    xf = x.detach().float().contiguous()
    y = torch.empty_like(xf)
    check(lib().mv_quant_float(_p(xf), _p(y), xf.numel(), exp_bits, man_bits, _s()), "quant_float", n=xf.numel())
    return y


def quant_float_f16(x):
    """float_quantize(x, exp=5, man=10) stored as IEEE half (exact) -- an operand of ``linear_f16``."""
    require_cuda(x)
    xf = x.detach().float().contiguous()
    y = torch.empty(xf.shape, dtype=torch.float16, device=xf.device)
    check(lib().mv_quant_float_f16(_p(xf), _p(y), xf.numel(), _s()), "quant_float_f16", n=xf.numel())
    return y


def linear_f16_supported(M, N, K):
    """Shapes the f16 MFMA GEMM takes (the 8-phase kernel: K % 128 == 0 and a grid worth a launch)."""
    return K % 128 == 0 and M >= 256 and N >= 256


def linear_f16(x16, w16, M, N, K, bias, out, residual=None):
    """out fp32 [M, N] = x16 [M, K] . w16 [N, K]^T + bias (+ residual): half operands on v_mfma_f32_16x16x32_f16, fp32
    accumulation."""
    epi, aux, ld_aux = (EPI_RESIDUAL, _p(residual), N) if residual is not None else (EPI_NONE, None, 0)
    with _timed("gemm_nt_f16", 2.0 * M * N * K, f"f16 N{N} K{K} epi{epi}"):
        check(lib().mv_gemm_nt_f16(_p(x16), K, _p(w16), K, _p(out), N, M, N, K, _p(bias), epi, aux, ld_aux, None, 0, _s()),
              "gemm_nt_f16", M=M, N=N, K=K)
    return out


def quant_fixed(x, wl, fl, clamp=True, symmetric=False):
    require_cuda(x)
    xf = x.detach().float().contiguous()
    y = torch.empty_like(xf)
    check(lib().mv_quant_fixed(_p(xf), _p(y), xf.numel(), wl, fl, int(clamp), int(symmetric), _s()), "quant_fixed",
          n=xf.numel())
    return y


def quant_affine(x, scale, zero_point, qmin, qmax):
    require_cuda(x)
    xf = x.detach().float().contiguous()
    y = torch.empty_like(xf)
    check(lib().mv_quant_affine(_p(xf), _p(y), xf.numel(), float(scale), int(zero_point), qmin, qmax, _s()),
          "quant_affine", n=xf.numel())
    return y


def quant_affine_codes(x, rows, cols, scale, zero_point, qmin, qmax, pre_gelu=False):
    """fp32 or bf16 [rows, cols] -> bf16 [rows, pad8(cols)] integer codes (q - zero_point) of the affine quantiser
    (exact); ``pre_gelu``: of gelu(x)."""
    require_cuda(x)
    xf = x.detach()
    if xf.dtype not in (torch.float32, torch.bfloat16):
        xf = xf.float()
    xf = xf.contiguous()
    ld = pad8(cols)
    codes = torch.empty(rows, ld, dtype=torch.bfloat16, device=x.device)
    check(lib().mv_quant_affine_codes(_p(xf), _DT[xf.dtype], _p(codes), rows, cols, ld, float(scale), int(zero_point), qmin,
                                      qmax, 1 if pre_gelu else 0, _s()),
          "quant_affine_codes", rows=rows, cols=cols)
    return codes


def linear_codes(xc, wc, M, N, K, alpha, bias, out, residual=None):
    """out (fp32 or bf16) [M, N] = alpha * (xc [M, pad8(K)] . wc [N, pad8(K)]^T) + bias (+ residual fp32 [M, N]):
    integer-code operands on the bf16 MFMA path = exact int8 arithmetic (|codes| <= 256, fp32 accumulation)."""
    epi, aux, ld_aux = (EPI_RESIDUAL, _p(residual), N) if residual is not None else (EPI_NONE, None, 0)
    with _timed("gemm_nt_bf16", 2.0 * M * N * K):
        check(lib().mv_gemm_nt_bf16_scaled(_p(xc), xc.shape[1], _p(wc), wc.shape[1], _p(out), N, _DT[out.dtype], M, N, K,
                                           float(alpha), _p(bias), epi, aux, ld_aux, 0, None, 0, _s()),
              "gemm_nt_bf16_scaled", M=M, N=N, K=K)
    return out


def pad16(n: int) -> int:
    return (n + 15) & ~15


def quant_affine_i8(x, rows, cols, scale, zero_point, pre_gelu=False):
    """fp32 or bf16 [rows, cols] -> int8 [rows, pad16(cols)] codes q - 128 of the quint8 affine quantiser (exact);
    ``pre_gelu``: of gelu(x).  Feeds ``linear_i8``."""
    require_cuda(x)
    xf = x.detach()
    if xf.dtype not in (torch.float32, torch.bfloat16):
        xf = xf.float()
    xf = xf.contiguous()
    ld = pad16(cols)
    codes = torch.empty(rows, ld, dtype=torch.int8, device=x.device)
    check(lib().mv_quant_affine_i8(_p(xf), _DT[xf.dtype], _p(codes), rows, cols, ld, float(scale), int(zero_point),
                                   1 if pre_gelu else 0, _s()), "quant_affine_i8", rows=rows, cols=cols)
    return codes


def linear_i8_supported(M, N, K):
    """Shapes the int8 MFMA GEMM takes (8-phase kernel: two whole 128-byte K-tiles per iteration, a grid worth a launch)."""
    return K % 256 == 0 and M >= 256 and N >= 256


def linear_i8(x8, w8, M, N, K, alpha, bias, icorr, out, residual=None, gelu_q8=None):
    """out (fp32 or bf16) [M, N] = alpha * (x8 [M, pad16(K)] . w8 [N, pad16(K)]^T + icorr[N]) + bias (+ residual fp32):
    int8 operands on v_mfma_i32_16x16x64_i8, int32 accumulation.  ``gelu_q8 = (scale, zero_point)`` of the NEXT layer's
    quint8 quantiser: ``out`` is int8 [M, N] and receives that quantiser's codes (q - 128) of gelu(the product)."""
    epi, aux, ld_aux = (EPI_RESIDUAL, _p(residual), N) if residual is not None else (EPI_NONE, None, 0)
    cdt, qs, qz = _DT.get(out.dtype), 0.0, 0
    if gelu_q8 is not None:
        if residual is not None or out.dtype != torch.int8:
            raise ValueError("gelu_q8 needs an int8 output and no residual")
        epi, cdt, qs, qz = _l.EPI_GELU_Q8, _l.MV_I8, float(gelu_q8[0]), int(gelu_q8[1])
    with _timed("gemm_nt_i8", 2.0 * M * N * K, f"i8 N{N} K{K} epi{epi}"):
        check(lib().mv_gemm_nt_i8(_p(x8), x8.shape[1], _p(w8), w8.shape[1], _p(out), N, cdt, M, N, K, float(alpha),
                                  _p(bias), _p(icorr), epi, aux, ld_aux, qs, qz, _s()), "gemm_nt_i8", M=M, N=N, K=K, epi=epi)
    return out


def layernorm_q8(x, ldx, rows, dim, gamma, beta, eps, scale, zero_point):
    """LayerNorm whose output goes straight into a quint8 quantiser: -> int8 codes (q - 128) [rows, dim]."""
    require_cuda(x, gamma, beta)
    codes = torch.empty(rows, dim, dtype=torch.int8, device=x.device)
    check(lib().mv_layernorm_fwd_q8(_p(x), ldx, _p(gamma), _p(beta), _p(codes), rows, dim, float(eps), float(scale),
                                    int(zero_point), _s()), "layernorm_fwd_q8", rows=rows, dim=dim)
    return codes


def minmax_update(x, state):
    """state: fp32 [4] on device, [0]=running min, [1]=running max (init +inf/-inf)."""
    require_cuda(x, state)                     # the kernel updates ``state`` with device atomics: never a host pointer
    if state.device != x.device or state.dtype != torch.float32 or not state.is_contiguous():
        raise RuntimeError("minmax_update: state must be a contiguous fp32 tensor on the input's device")
    xf = x.detach().float().contiguous()
    check(lib().mv_minmax(_p(xf), xf.numel(), _p(state), _s()), "minmax", n=xf.numel())


# ------------------------------------------------------------------------------------------------------------
# loss, upsample, optimizer
# ------------------------------------------------------------------------------------------------------------
def cross_entropy(logits, labels, *, want_grad, grad_dtype=torch.float32, ld_dl=None, want_argmax=False):
    """Mean CE.  logits fp32 [B, C] or [B, C, H, W]; labels int64.  -> (loss[1], dlogits|None, argmax|None)"""
    require_cuda(logits, labels)
    logits = logits.contiguous()
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    C = logits.shape[1]
    outer = logits.shape[0]
    inner = 1
    for s in logits.shape[2:]:
        inner *= s
    stat = torch.empty(4, dtype=torch.float32, device=logits.device)   # mean loss, counted labels, bad labels, unused
    loss = stat[:1]
    dl = None
    if want_grad:
        if inner == 1:
            ld_dl = C if ld_dl is None else ld_dl
            dl = torch.empty(outer, ld_dl, dtype=grad_dtype, device=logits.device)
        else:
            ld_dl = C
            dl = torch.empty(logits.shape, dtype=grad_dtype, device=logits.device)
    am = torch.empty(labels.shape, dtype=torch.int64, device=logits.device) if want_argmax else None
    check(lib().mv_cross_entropy(_p(logits), _p(labels), _p(stat), _p(dl), _DT[grad_dtype], ld_dl or C, _p(am), outer, C,
                                 inner, 1.0, _s()), "cross_entropy", outer=outer, C=C, inner=inner)
    return loss, dl, am


def cross_entropy_soft(logits, labels, lam=1.0, smoothing=0.0, pair_flip=True, want_grad=False, want_argmax=False,
                       grad_scale=1.0):
    """Mean soft-target CE of Mixup / CutMix and label smoothing (mv_cross_entropy_soft): logits fp32 [B, C], labels int64 [B];
    sample i is paired with B-1-i and its target is ``lam * s(y_i) + (1-lam) * s(y_j)``, ``s`` = one-hot smoothed by ``smoothing``.
    ``lam`` is a host scalar.  -> (loss[1], dlogits|None, argmax|None, per-sample losses [B])"""
    require_cuda(logits, labels)
    if logits.dim() != 2 or labels.shape != logits.shape[:1]:
        raise RuntimeError(f"cross_entropy_soft: logits [B, C] and labels [B] expected, got {tuple(logits.shape)} and "
                           f"{tuple(labels.shape)}")
    if logits.dtype != torch.float32:
        raise RuntimeError("cross_entropy_soft: fp32 logits expected")
    logits = logits.contiguous()
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    B, C = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    per_sample = torch.empty(B, dtype=torch.float32, device=logits.device)
    dl = torch.empty(B, C, dtype=torch.float32, device=logits.device) if want_grad else None
    am = torch.empty(B, dtype=torch.int64, device=logits.device) if want_argmax else None
    check(lib().mv_cross_entropy_soft(_p(logits), _p(labels), _p(loss), _p(per_sample), _p(dl), _p(am), B, C, float(lam),
                                      float(smoothing), int(bool(pair_flip)), float(grad_scale), _s()),
          "cross_entropy_soft", B=B, C=C, lam=lam, smoothing=smoothing, pair_flip=bool(pair_flip))
    return loss, dl, am, per_sample


DISTILL_MODES = {"soft": 0, "hard": 1}          # MV_DISTILL_SOFT / MV_DISTILL_HARD


def distill_loss(student, distill, teacher, labels, temperature=1.0, alpha=0.5, mode="soft", lam=1.0, smoothing=0.0,
                 pair_flip=False, want_grad=False, want_argmax=False, grad_scale=1.0):
    """DeiT distillation loss (mv_distill_loss; models/distill.py:142-151): ``alpha * CE(student, labels) + (1 - alpha) * KD`` with
    ``KD = T^2 * kl_div(log_softmax(distill / T), softmax(teacher / T), "batchmean")`` (``mode="soft"``) or the cross entropy of the
    distillation logits against the teacher's arg-max (``"hard"``).  All three logits fp32 [B, C], labels int64 [B]; the cross
    entropy takes ``lam`` / ``smoothing`` / ``pair_flip`` as ``cross_entropy_soft`` does.  Host scalars throughout.
    -> (loss [3] = total | CE mean | KD mean, dstudent|None, ddistill|None, argmax|None, per-sample losses [2, B])"""
    require_cuda(student, distill, teacher, labels)
    if mode not in DISTILL_MODES:
        raise ValueError(f"distillation_type must be 'soft' or 'hard', got {mode!r}")
    if student.dim() != 2 or distill.shape != student.shape or teacher.shape != student.shape or labels.shape != student.shape[:1]:
        raise RuntimeError(f"distill_loss: three [B, C] logits and labels [B] expected, got {tuple(student.shape)}, "
                           f"{tuple(distill.shape)}, {tuple(teacher.shape)} and {tuple(labels.shape)}")
    if not (student.dtype == distill.dtype == teacher.dtype == torch.float32):
        raise RuntimeError("distill_loss: fp32 logits expected")
    student, distill, teacher, labels = student.contiguous(), distill.contiguous(), teacher.contiguous(), labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    B, C = student.shape
    dev = student.device
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    per_sample = torch.empty(2, B, dtype=torch.float32, device=dev)
    ds = torch.empty(B, C, dtype=torch.float32, device=dev) if want_grad else None
    dd = torch.empty(B, C, dtype=torch.float32, device=dev) if want_grad else None
    am = torch.empty(B, dtype=torch.int64, device=dev) if want_argmax else None
    check(lib().mv_distill_loss(_p(student), _p(distill), _p(teacher), _p(labels), _p(loss), _p(per_sample), _p(ds), _p(dd), _p(am),
                                B, C, DISTILL_MODES[mode], float(temperature), float(alpha), float(lam), float(smoothing),
                                int(bool(pair_flip)), float(grad_scale), _s()),
          "distill_loss", B=B, C=C, mode=mode, temperature=temperature, alpha=alpha, lam=lam, smoothing=smoothing,
          pair_flip=bool(pair_flip))
    return loss, ds, dd, am, per_sample


def mix_batch(x, *, lam=None, box=None):
    """Mixup (``lam``) or CutMix (``box`` = (y0, y1, x0, x1)) of a dense [B, Ch, H, W] fp32 / bf16 batch IN PLACE
    (mv_mix_batch): sample i with sample B-1-i.  Both arguments are host scalars.  -> x"""
    require_cuda(x)
    if (lam is None) == (box is None):
        raise ValueError("mix_batch: exactly one of lam (Mixup) and box (CutMix) is given")
    if x.dim() != 4 or not x.is_contiguous() or x.dtype not in _DT:
        raise RuntimeError("mix_batch: a contiguous [B, Ch, H, W] fp32 or bf16 batch expected "
                           f"(got {tuple(x.shape)}, {x.dtype}, contiguous={x.is_contiguous()})")
    B, Ch, H, W = x.shape
    mode, y0, y1, x0, x1 = (0, 0, 0, 0, 0) if box is None else (1, *(int(v) for v in box))
    check(lib().mv_mix_batch(_p(x), _DT[x.dtype], B, Ch, H, W, mode, 1.0 if lam is None else float(lam), y0, y1, x0, x1, _s()),
          "mix_batch", B=B, Ch=Ch, H=H, W=W, mode=mode, lam=lam, box=box)
    return x


def upsample_bilinear_fwd(small, sb, sc, sp, B, C, h, w, H, W):
    big = torch.empty(B, C, H, W, dtype=torch.float32, device=small.device)
    check(lib().mv_upsample_bilinear_fwd(_p(small), sb, sc, sp, _p(big), B, C, h, w, H, W, _s()), "upsample_fwd",
          B=B, C=C, h=h, w=w, H=H, W=W)
    return big


def upsample_bilinear_bwd(dbig, dsmall, sb, sc, sp, B, C, h, w, H, W):
    check(lib().mv_upsample_bilinear_bwd(_p(dbig), _p(dsmall), sb, sc, sp, B, C, h, w, H, W, _s()), "upsample_bwd",
          B=B, C=C, h=h, w=w, H=H, W=W)
    return dsmall


SEG_CE_MAX_CLASSES = 32
SEG_CE_LDS_LIMIT = 64 * 1024


def seg_ce_supported(C, h, w, W):
    """Shapes the fused segmentation tail covers (mv_seg_ce_* return MV_ERR_UNSUPPORTED outside them)."""
    return C <= SEG_CE_MAX_CLASSES and (h * w * C + W * C) * 4 <= SEG_CE_LDS_LIMIT


def seg_ce_fwd(small, labels, B, C, h, w, H, W):
    """small fp32 [B*h*w, C], labels int64 [B,H,W] -> (stats[2] = mean loss, pixel accuracy; lse [B,H,W]; pred u8)."""
    require_cuda(small, labels)
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    dev = small.device
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    nblk = lib().mv_seg_ce_partials(B, H, W)
    partials = torch.empty(max(4 * nblk, 4), dtype=torch.float32, device=dev)
    stats = torch.empty(4, dtype=torch.float32, device=dev)      # mean loss, pixel accuracy, counted labels, bad labels
    check(lib().mv_seg_ce_fwd(_p(small), _p(labels), _p(lse), _p(pred), _p(partials), _p(stats), B, C, h, w, H, W, _s()),
          "seg_ce_fwd", B=B, C=C, h=h, w=w, H=H, W=W)
    return stats, lse, pred, labels


def seg_ce_bwd(small, labels, lse, B, C, h, w, H, W, *, grad_dtype=torch.float32, ld=None, grad_scale=1.0, stats=None):
    """``stats``: the forward's (its label count is the mean's denominator); None = every pixel counts."""
    ld = C if ld is None else ld
    ds = torch.empty(B * h * w, ld, dtype=grad_dtype, device=small.device)
    check(lib().mv_seg_ce_bwd(_p(small), _p(labels), _p(lse), _p(stats), _p(ds), _DT[grad_dtype], ld, grad_scale, B, C, h, w,
                              H, W, _s()), "seg_ce_bwd", B=B, C=C, h=h, w=w, H=H, W=W, ld=ld)
    return ds


SEG_LOSS_MAX_CLASSES = 32
SEG_LOSS_FWD_EXTRA, SEG_LOSS_BWD_EXTRA = 400, 128          # LDS words behind the map: csrc/seg_loss.hip SL_FWD_EXTRA / SL_BWD_EXTRA


def seg_loss_supported(C, h, w, W):
    """Shapes the fused segmentation tail WITH a recipe covers (mv_seg_loss_* return MV_ERR_UNSUPPORTED outside them)."""
    return (C <= SEG_LOSS_MAX_CLASSES and (h * w * C + SEG_LOSS_FWD_EXTRA) * 4 <= SEG_CE_LDS_LIMIT
            and (h * w * C + W * C + SEG_LOSS_BWD_EXTRA) * 4 <= SEG_CE_LDS_LIMIT)


def seg_loss_fwd(small, labels, B, C, h, w, H, W, *, class_weight=None, label_smoothing=0.0, dice_weight=0.0, dice_smooth=1.0,
                 areas=True):
    """small fp32 [B*h*w, C], labels int64 [B,H,W], class_weight fp32 [C] on the device or None (ones) ->
    (stats [8] = loss, pixel accuracy, counted labels, bad labels, CE, Dice, sum of w_y, 0; lse [B,H,W]; pred u8 [B,H,W];
    coef [2, C] = (a_c, b_c) of the Dice gradient; areas int64 [3, C] = (intersect, pred, label) or None; labels as read)."""
    require_cuda(small, labels)
    labels = labels.contiguous()
    if labels.dtype != torch.int64:
        labels = labels.long()
    if class_weight is not None:
        require_cuda(class_weight)
        if class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (C,) or not class_weight.is_contiguous():
            raise RuntimeError(f"seg_loss_fwd: class_weight must be a contiguous fp32 [{C}] tensor")
    dev = small.device
    lse = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    partials = torch.empty(max(lib().mv_seg_loss_partials(B, C, H, W), 4), dtype=torch.float32, device=dev)
    stats = torch.empty(8, dtype=torch.float32, device=dev)
    coef = torch.empty(2, C, dtype=torch.float32, device=dev)
    ar = torch.empty(3, C, dtype=torch.int64, device=dev) if areas else None
    check(lib().mv_seg_loss_fwd(_p(small), _p(labels), _p(class_weight), label_smoothing, dice_weight, dice_smooth, _p(lse), _p(pred),
                                _p(partials), _p(stats), _p(coef), _p(ar), B, C, h, w, H, W, _s()),
          "seg_loss_fwd", B=B, C=C, h=h, w=w, H=H, W=W, label_smoothing=label_smoothing, dice_weight=dice_weight,
          dice_smooth=dice_smooth)
    return stats, lse, pred, coef, ar, labels


def seg_loss_bwd(small, labels, lse, stats, coef, B, C, h, w, H, W, *, class_weight=None, label_smoothing=0.0, dice_weight=0.0,
                 grad_dtype=torch.float32, ld=None, grad_scale=1.0):
    """``stats`` and ``coef``: the forward's.  -> d(loss)/d(small) * grad_scale, ``grad_dtype`` [B*h*w, ld]."""
    ld = C if ld is None else ld
    ds = torch.empty(B * h * w, ld, dtype=grad_dtype, device=small.device)
    check(lib().mv_seg_loss_bwd(_p(small), _p(labels), _p(class_weight), label_smoothing, dice_weight, _p(lse), _p(stats), _p(coef),
                                _p(ds), _DT[grad_dtype], ld, grad_scale, B, C, h, w, H, W, _s()),
          "seg_loss_bwd", B=B, C=C, h=h, w=w, H=H, W=W, ld=ld, label_smoothing=label_smoothing, dice_weight=dice_weight)
    return ds


# ------------------------------------------------------------------------------------------------------------
# YOLOS detection tail (csrc/detection.hip): fp32 in every precision
# ------------------------------------------------------------------------------------------------------------
def _f32c(t):
    t = t.detach()
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def det_heads_fwd(x, w_cls, b_cls, w_box, b_box, Q):
    """x fp32 [B, T, D] -> (logits [B, Q, C1], boxes [B, Q, 4] after the sigmoid) from the last Q rows of every image."""
    require_cuda(x, w_cls, b_cls, w_box, b_box)
    B, T, D = x.shape
    C1 = w_cls.shape[0]
    logits = torch.empty(B, Q, C1, dtype=torch.float32, device=x.device)
    boxes = torch.empty(B, Q, 4, dtype=torch.float32, device=x.device)
    check(lib().mv_det_heads_fwd(_p(x), _p(w_cls), _p(b_cls), _p(w_box), _p(b_box), _p(logits), _p(boxes), B, T, Q, D, C1, _s()),
          "det_heads_fwd", B=B, T=T, Q=Q, D=D, C1=C1)
    return logits, boxes


def det_heads_bwd(x, w_cls, w_box, boxes, dlogits, dboxes, Q, *, want_dx=True, params=(None, None, None, None)):
    """-> (dx [B, T, D] or None, dw_cls, db_cls, dw_box, db_box); ``params``: the four parameters (gradient destinations)."""
    B, T, D = x.shape
    C1 = w_cls.shape[0]
    dev = x.device
    dx = torch.zeros_like(x) if want_dx else None                # the kernel writes the last Q rows of every image
    dwc, dbc = grad_out(params[0], (C1, D), dev), grad_out(params[1], (C1,), dev)
    dwb, dbb = grad_out(params[2], (4, D), dev), grad_out(params[3], (4,), dev)
    ws = workspace(lib().mv_det_heads_bwd_workspace_bytes(B, Q, D, C1), dev)
    check(lib().mv_det_heads_bwd(_p(x), _p(w_cls), _p(w_box), _p(boxes), _p(dlogits), _p(dboxes), _p(dx), _p(dwc), _p(dbc),
                                 _p(dwb), _p(dbb), _p(ws), ws.numel(), B, T, Q, D, C1, _s()),
          "det_heads_bwd", B=B, T=T, Q=Q, D=D, C1=C1)
    return dx, dwc, dbc, dwb, dbb


def det_append_fwd(x, det, pos):
    """cat(x [B, T0, D], det [Q, D] + pos [Q, D]) -> [B, T0 + Q, D]."""
    require_cuda(x, det, pos)
    B, T0, D = x.shape
    Q = det.shape[0]
    out = torch.empty(B, T0 + Q, D, dtype=torch.float32, device=x.device)
    check(lib().mv_det_append_fwd(_p(x), _p(det), _p(pos), _p(out), B, T0, Q, D, _s()), "det_append_fwd", B=B, T0=T0, Q=Q, D=D)
    return out


def det_append_bwd(dout, T0, Q, det=None, pos=None):
    """dout [B, T0 + Q, D] -> (dx [B, T0, D], ddet [Q, D], dpos [Q, D])."""
    B, T, D = dout.shape
    dx = torch.empty(B, T0, D, dtype=torch.float32, device=dout.device)
    ddet, dpos = grad_out(det, (Q, D), dout.device), grad_out(pos, (Q, D), dout.device)
    check(lib().mv_det_append_bwd(_p(dout), _p(dx), _p(ddet), _p(dpos), B, T0, Q, D, _s()), "det_append_bwd", B=B, T0=T0, Q=Q,
          D=D)
    return dx, ddet, dpos


def det_cost(logits, boxes, labels, tboxes, toff, total, cost_class, cost_bbox, cost_giou):
    """Packed per-image cost blocks: fp32 [Q * total]; the [Q, T_b] block of image b starts at Q * toff[b]."""
    require_cuda(logits, boxes, labels, tboxes, toff)
    B, Q, C1 = logits.shape
    out = torch.empty(Q * total, dtype=torch.float32, device=logits.device)
    if total > 0:
        check(lib().mv_det_cost(_p(logits), _p(boxes), _p(labels), _p(tboxes), _p(toff), _p(out), float(cost_class),
                                float(cost_bbox), float(cost_giou), B, Q, C1, _s()), "det_cost", B=B, Q=Q, C1=C1)
    return out


DET_MATCH_MAX = 1024          # mv_det_match: the largest Q and T_b one wave's LDS state holds


def det_match(cost, toff, B, Q, max_t):
    """Packed cost blocks (``det_cost``) -> (match int32 [B * Q]: flat target index of every query or -1, status int32 [B]:
    0 solved, 1 NaN / -inf in the block or a target count outside [0, ``max_t``], 2 infeasible; an image with a non-zero status has
    -1 throughout).  ``max_t``: the largest target count.  No host copy."""
    require_cuda(cost, toff)
    match = torch.empty(B * Q, dtype=torch.int32, device=cost.device)
    status = torch.empty(B, dtype=torch.int32, device=cost.device)
    check(lib().mv_det_match(_p(cost), _p(toff), _p(match), _p(status), B, Q, max_t, _s()), "det_match", B=B, Q=Q, max_t=max_t)
    return match, status


def det_assign(match, labels, tboxes, B, Q, no_object):
    """match int32 [B * Q] (flat target index or -1) -> (tgt_class int64 [B, Q], tgt_box fp32 [B, Q, 4])."""
    require_cuda(match, labels, tboxes)
    tgt_class = torch.empty(B, Q, dtype=torch.int64, device=match.device)
    tgt_box = torch.empty(B, Q, 4, dtype=torch.float32, device=match.device)
    check(lib().mv_det_assign(_p(match), _p(labels), _p(tboxes), _p(tgt_class), _p(tgt_box), B * Q, labels.numel(), no_object,
                              _s()), "det_assign", B=B, Q=Q)
    return tgt_class, tgt_box


def det_loss_fwd(logits, boxes, tgt_class, tgt_box, weight, tcount, num_boxes):
    """-> (stats fp32 [8]: loss_ce, loss_bbox, loss_giou, class_error, cardinality_error, sum of weights, matched, bad; lse)."""
    require_cuda(logits, boxes, tgt_class, tgt_box, weight, tcount)
    B, Q, C1 = logits.shape
    stats = torch.empty(8, dtype=torch.float32, device=logits.device)
    lse = torch.empty(B * Q, dtype=torch.float32, device=logits.device)
    check(lib().mv_det_loss_fwd(_p(logits), _p(boxes), _p(tgt_class), _p(tgt_box), _p(weight), _p(tcount), _p(lse), _p(stats),
                                1.0 / num_boxes, B, Q, C1, _s()), "det_loss_fwd", B=B, Q=Q, C1=C1)
    return stats, lse


def det_loss_bwd(logits, boxes, tgt_class, tgt_box, weight, lse, stats, g_ce, g_bbox, g_giou, num_boxes):
    B, Q, C1 = logits.shape
    dlogits, dboxes = torch.empty_like(logits), torch.empty_like(boxes)
    check(lib().mv_det_loss_bwd(_p(logits), _p(boxes), _p(tgt_class), _p(tgt_box), _p(weight), _p(lse), _p(stats), _p(g_ce),
                                _p(g_bbox), _p(g_giou), _p(dlogits), _p(dboxes), 1.0 / num_boxes, B, Q, C1, _s()),
          "det_loss_bwd", B=B, Q=Q, C1=C1)
    return dlogits, dboxes


def det_postprocess(logits, boxes, sizes):
    """-> (scores [B, Q], labels int64 [B, Q], boxes xyxy scaled by (w, h, w, h) [B, Q, 4]); sizes [B, 2] = (height, width)."""
    require_cuda(logits, boxes, sizes)
    B, Q, C1 = logits.shape
    scores = torch.empty(B, Q, dtype=torch.float32, device=logits.device)
    labels = torch.empty(B, Q, dtype=torch.int64, device=logits.device)
    out = torch.empty(B, Q, 4, dtype=torch.float32, device=logits.device)
    check(lib().mv_det_postprocess(_p(logits), _p(boxes), _p(sizes), _p(scores), _p(labels), _p(out), B, Q, C1, _s()),
          "det_postprocess", B=B, Q=Q, C1=C1)
    return scores, labels, out


def image_prepare(raw, kh, bh, kv, bv, flip, mean, std):
    """uint8 [B, Hs, Ws, 3] + Pillow resampling tables -> fp32 [B, 3, oh, ow] (crop/resize/flip/ToTensor/Normalize)."""
    require_cuda(raw, kh, bh, kv, bv, flip)
    B, Hs, Ws, _ = raw.shape
    oh, ow, ks = kv.shape[1], kh.shape[1], kh.shape[2]
    out = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=raw.device)
    check(lib().mv_image_prepare(_p(raw), Hs * Ws * 3, Hs, Ws, _p(kh), _p(bh), _p(kv), _p(bv), ks, _p(flip),
                                 mean[0], mean[1], mean[2], std[0], std[1], std[2], _p(out), B, oh, ow, _s()),
          "image_prepare", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow, ks=ks)
    return out


def image_resize_u8(raw, kh, bh, kv, bv):
    """uint8 [B, Hs, Ws, 3] + Pillow resampling tables -> uint8 [B, oh, ow, 3]: a plain Image.resize(BILINEAR), kept as
    the uint8 image a following RandomResizedCrop resamples again."""
    require_cuda(raw, kh, bh, kv, bv)
    B, Hs, Ws, _ = raw.shape
    oh, ow, ks = kv.shape[1], kh.shape[1], kh.shape[2]
    out = torch.empty(B, oh, ow, 3, dtype=torch.uint8, device=raw.device)
    check(lib().mv_image_resize_u8(_p(raw), Hs * Ws * 3, Hs, Ws, _p(kh), _p(bh), _p(kv), _p(bv), ks, _p(out), B, oh, ow, _s()),
          "image_resize_u8", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow, ks=ks)
    return out


def _ragged_out(out, shape, dtype, device):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"output must be a contiguous {dtype} tensor of shape {tuple(shape)}")
    require_cuda(out)
    return out


def image_prepare_ragged(raw, kh, bh, kv, bv, ext, mean, std, out=None, mask=None):
    """uint8 [B, Hs, Ws, 3] + per-sample tables padded to [B, ow, ks] / [B, oh, ks] + extents int32 [B, 2] = (oh_b, ow_b) ->
    (fp32 [B, 3, oh, ow], zero outside each sample's extent; bool [B, oh, ow] padding mask, True = padding).  ``out`` / ``mask``:
    preallocated results (every element is written)."""
    require_cuda(raw, kh, bh, kv, bv, ext)
    B, Hs, Ws, _ = raw.shape
    oh, ow, ks = kv.shape[1], kh.shape[1], kh.shape[2]
    if kv.shape[2] != ks or ext.shape != (B, 2) or ext.dtype != torch.int32:
        raise ValueError("image_prepare_ragged: tables must share the tap count and ext must be int32 [B, 2]")
    out = _ragged_out(out, (B, 3, oh, ow), torch.float32, raw.device)
    mask = _ragged_out(mask, (B, oh, ow), torch.bool, raw.device)
    check(lib().mv_image_prepare_ragged(_p(raw), Hs * Ws * 3, Hs, Ws, _p(kh), _p(bh), _p(kv), _p(bv), ks, _p(ext),
                                        mean[0], mean[1], mean[2], std[0], std[1], std[2], _p(out), _p(mask), B, oh, ow, _s()),
          "image_prepare_ragged", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow, ks=ks)
    return out, mask


def image_resize_u8_ragged(raw, kh, bh, kv, bv, ext, out=None):
    """The uint8 intermediate of a two-resampling chain for a ragged batch -> uint8 [B, oh, ow, 3], zeros outside the extents."""
    require_cuda(raw, kh, bh, kv, bv, ext)
    B, Hs, Ws, _ = raw.shape
    oh, ow, ks = kv.shape[1], kh.shape[1], kh.shape[2]
    if kv.shape[2] != ks or ext.shape != (B, 2) or ext.dtype != torch.int32:
        raise ValueError("image_resize_u8_ragged: tables must share the tap count and ext must be int32 [B, 2]")
    out = _ragged_out(out, (B, oh, ow, 3), torch.uint8, raw.device)
    check(lib().mv_image_resize_u8_ragged(_p(raw), Hs * Ws * 3, Hs, Ws, _p(kh), _p(bh), _p(kv), _p(bv), ks, _p(ext), _p(out),
                                          B, oh, ow, _s()),
          "image_resize_u8_ragged", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow, ks=ks)
    return out


def mask_resize_u8(mask, yi, xi):
    """uint8 [B, Hs, Ws] + NEAREST index tables -> uint8 [B, oh, ow]."""
    require_cuda(mask, yi, xi)
    B, Hs, Ws = mask.shape
    oh, ow = yi.shape[1], xi.shape[1]
    out = torch.empty(B, oh, ow, dtype=torch.uint8, device=mask.device)
    check(lib().mv_mask_resize_u8(_p(mask), Hs * Ws, Hs, Ws, _p(yi), _p(xi), _p(out), B, oh, ow, _s()),
          "mask_resize_u8", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow)
    return out


def mask_prepare(mask, yi, xi, flip, add=0):
    """uint8 [B, Hs, Ws] + NEAREST index tables -> int64 [B, oh, ow] (+ add)."""
    require_cuda(mask, yi, xi, flip)
    B, Hs, Ws = mask.shape
    oh, ow = yi.shape[1], xi.shape[1]
    out = torch.empty(B, oh, ow, dtype=torch.int64, device=mask.device)
    check(lib().mv_mask_prepare(_p(mask), Hs * Ws, Hs, Ws, _p(yi), _p(xi), _p(flip), add, _p(out), B, oh, ow, _s()),
          "mask_prepare", B=B, Hs=Hs, Ws=Ws, oh=oh, ow=ow)
    return out


def adamw_step(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, clip_coef=None, hyper=None):
    """In-place AdamW on flat fp32 tensors (torch.optim.AdamW semantics).  ``clip_coef``: fp32 device scalar multiplied
    into every gradient (``grad_norm_clip``).  ``hyper`` (fp32 [3] on the device: lr, 1 - beta1^step, 1 - beta2^step)
    replaces ``lr`` / ``step``: what a launch captured in a HIP graph reads, see ``utils.optim.AdamW.use_device_scalars``."""
    require_cuda(p, g, m, v, clip_coef, hyper)
    if hyper is not None:
        check(lib().mv_adamw_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), beta1, beta2, eps, weight_decay, grad_scale,
                                 _p(clip_coef), _s()), "adamw_dev", n=p.numel())
        return
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    check(lib().mv_adamw(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, bc1, bc2,
                         grad_scale, _p(clip_coef), _s()), "adamw", n=p.numel())


def adamw_table_step(p, g, m, v, items, seg_lr_scale, seg_wd, *, lr, beta1, beta2, eps, step, grad_scale=1.0, clip_coef=None,
                     hyper=None, ema=None, ema_decay=0.0):
    """In-place AdamW over a whole flat fp32 arena in ONE launch (``mv_adamw_table``).  ``items`` = (offsets int64 [n], lengths
    int32 [n], segments int32 [n]) on the device, cut by ``utils.optim.build_items``; ``seg_lr_scale`` / ``seg_wd`` fp32 [n_seg]:
    element i of an item of segment s steps at ``lr * seg_lr_scale[s]`` with weight decay ``seg_wd[s]``.  ``clip_coef`` and ``hyper``
    as in ``adamw_step``.  ``ema`` (fp32, shaped like ``p``): ``ema = ema_decay * ema + (1 - ema_decay) * p_new`` in the same pass."""
    require_cuda(p, g, m, v, *items, seg_lr_scale, seg_wd, clip_coef, hyper, ema)
    item_ptrs, n_items, seg_args = _table_args("adamw_table_step", (p, g, m, v, ema), items, seg_lr_scale, seg_wd)
    lr, bc1, bc2 = _launch_scalars(hyper, lr, (beta1, beta2), step)
    check(lib().mv_adamw_table(_p(p), _p(g), _p(m), _p(v), _p(ema), *item_ptrs, n_items, *seg_args, _p(hyper), lr, beta1, beta2, eps,
                               bc1, bc2, grad_scale, _p(clip_coef), float(ema_decay), _s()), "adamw_table", n=p.numel(), items=n_items)


def _table_args(op, arrays, items, seg_lr_scale, seg_wd):
    """The argument checks of every step on the work list, and the arguments they all pass -> (pointers to the item offsets, lengths
    and segments), the item count, (pointers to ``seg_lr_scale`` and ``seg_wd``, the segment count)."""
    off, length, seg = items
    if not (off.dtype == torch.int64 and length.dtype == torch.int32 and seg.dtype == torch.int32
            and off.numel() == length.numel() == seg.numel()):
        raise ValueError(f"{op}: items are (int64 offsets, int32 lengths, int32 segments) of one length")
    present = [a for a in arrays if a is not None]
    if any(a.dtype != torch.float32 or a.numel() != present[0].numel() for a in present):
        raise ValueError(f"{op}: the parameter, gradient, state (and ema) arrays must be fp32 of one size")
    if seg_lr_scale.dtype != torch.float32 or seg_wd.dtype != torch.float32 or seg_lr_scale.numel() != seg_wd.numel():
        raise ValueError(f"{op}: seg_lr_scale and seg_wd are fp32 tables of one length")
    return (_p(off), _p(length), _p(seg)), off.numel(), (_p(seg_lr_scale), _p(seg_wd), seg_wd.numel())


def _launch_scalars(hyper, lr, betas=(0.0, 0.0), step=1):
    """-> (lr, 1 - beta1^step, 1 - beta2^step) as launch arguments; 0.0 / 1.0 / 1.0 when ``hyper`` holds them on the device."""
    return (0.0, 1.0, 1.0) if hyper is not None else (lr, 1.0 - betas[0] ** step, 1.0 - betas[1] ** step)


def sgd_table_step(p, g, buf, items, seg_lr_scale, seg_wd, *, lr, momentum, nesterov, grad_scale=1.0, clip_coef=None, hyper=None,
                   ema=None, ema_decay=0.0):
    """In-place SGD over a whole flat fp32 arena in ONE launch (``mv_sgd_table``; ``torch.optim.SGD`` with dampening 0).  ``items``,
    ``seg_lr_scale`` / ``seg_wd``, ``clip_coef``, ``hyper`` (only its first entry, the rate, is read) and ``ema`` as in
    ``adamw_table_step``.  ``buf``: the momentum buffer, shaped like ``p``; None with ``momentum == 0`` (nothing is read or written)."""
    require_cuda(p, g, buf, *items, seg_lr_scale, seg_wd, clip_coef, hyper, ema)
    item_ptrs, n_items, seg_args = _table_args("sgd_table_step", (p, g, buf, ema), items, seg_lr_scale, seg_wd)
    if (buf is None) != (momentum == 0):
        raise ValueError("sgd_table_step: a momentum buffer goes with momentum != 0, and only with it")
    check(lib().mv_sgd_table(_p(p), _p(g), _p(buf), _p(ema), *item_ptrs, n_items, *seg_args, _p(hyper), _launch_scalars(hyper, lr)[0],
                             momentum, int(bool(nesterov)), grad_scale, _p(clip_coef), float(ema_decay), _s()), "sgd_table",
          n=p.numel(), items=n_items)


def lamb_workspace(n_items, device):
    """The per-item partial sums of ``lamb_table_step`` (two doubles per item): allocated ONCE by the optimizer that steps with it, so
    that a captured step replays on the same memory.  Needs no initialisation."""
    return torch.empty(max(1, lib().mv_lamb_workspace_bytes(int(n_items)) // 8), dtype=torch.float64, device=device)


def lamb_table_step(p, g, m, v, items, item_tensor, tensor_range, seg_lr_scale, seg_wd, workspace, *, lr, beta1, beta2, eps, step,
                    grad_scale=1.0, clip_coef=None, hyper=None, ema=None, ema_decay=0.0):
    """In-place LAMB over a whole flat fp32 arena in TWO launches (``mv_lamb_table``): the moments and one pair of partial sums per
    item, then per item the trust ratio ``||p|| / ||u||`` of its tensor and the step.  ``item_tensor`` (int32 [n_items]) and
    ``tensor_range`` (int32 [n_tensors, 2]: first item, item count) from ``utils.optim.build_item_tensors``; ``workspace`` from
    ``lamb_workspace``; everything else as in ``adamw_table_step``."""
    require_cuda(p, g, m, v, *items, item_tensor, tensor_range, seg_lr_scale, seg_wd, workspace, clip_coef, hyper, ema)
    item_ptrs, n_items, seg_args = _table_args("lamb_table_step", (p, g, m, v, ema), items, seg_lr_scale, seg_wd)
    if not (item_tensor.dtype == torch.int32 and item_tensor.numel() == n_items and tensor_range.dtype == torch.int32
            and tensor_range.dim() == 2 and tensor_range.shape[1] == 2 and tensor_range.is_contiguous()):
        raise ValueError("lamb_table_step: item_tensor is int32 [n_items], tensor_range int32 [n_tensors, 2]")
    if workspace.dtype != torch.float64 or workspace.numel() < 2 * n_items:
        raise ValueError("lamb_table_step: the workspace holds two doubles per item (lamb_workspace)")
    lr, bc1, bc2 = _launch_scalars(hyper, lr, (beta1, beta2), step)
    check(lib().mv_lamb_table(_p(p), _p(g), _p(m), _p(v), _p(ema), *item_ptrs, _p(item_tensor), n_items, _p(tensor_range),
                              tensor_range.shape[0], *seg_args, _p(hyper), lr, beta1, beta2, eps, bc1, bc2, grad_scale, _p(clip_coef),
                              float(ema_decay), _p(workspace), workspace.numel() * 8, _s()), "lamb_table", n=p.numel(), items=n_items)


def grad_norm_clip(g, max_norm, grad_scale=1.0):
    """-> fp32 [2] on the device: (total_norm of g * grad_scale, min(1, max_norm / (total_norm + 1e-6))) -- the two numbers
    of torch.nn.utils.clip_grad_norm_ (classification/train.py:265-270); no host synchronisation."""
    require_cuda(g)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    ws = workspace(lib().mv_grad_norm_workspace_bytes(), g.device)
    check(lib().mv_grad_norm_clip(_p(g), g.numel(), float(grad_scale), float(max_norm), _p(out), _p(ws), ws.numel(), _s()),
          "grad_norm_clip", n=g.numel())
    return out


def dropout(x, p, seed, offset, out=None):
    """x * keep / (1 - p) with the Philox mask of (seed, offset); fp32 or bf16, any shape (contiguous)."""
    require_cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x) if out is None else out
    check(lib().mv_dropout(_p(x), _p(y), _DT[x.dtype], x.numel(), float(p), int(seed), int(offset), _s()), "dropout",
          n=x.numel(), p=p)
    return y


# ------------------------------------------------------------------------------------------------------------
# stochastic depth (drop path): one factor per sample and residual branch
# ------------------------------------------------------------------------------------------------------------
DROP_PATH_THREADS = 256           # threads per workgroup of mv_drop_path_add / mv_row_scale, one 16-byte vector each per grid pass
DROP_PATH_MAX_BLOCKS_PER_CU = 8   # their grid never exceeds this many workgroups per compute unit (csrc/drop_path.hip)


def drop_path_tables(rates):
    """(thr, scale) of ``mv_drop_path_draw`` for drop rates ``rates`` (each in [0, 1)), computed in double on the host:
    thr[r] = int(p_r * 2**32) as a python int, scale[r] = 1 / (1 - p_r) as a python float (the caller rounds it to fp32)."""
    for p in rates:
        if not 0.0 <= p < 1.0:
            raise ValueError(f"drop path rate has to be in [0, 1), got {p}")
    return [int(float(p) * 4294967296.0) for p in rates], [1.0 / (1.0 - float(p)) for p in rates]


def drop_path_draw(state, thr, scale, B):
    """One launch: a fresh fp32 [R, B] table of per-sample factors (0 or scale[r]) from the Philox stream of ``state`` (device
    int64[2] = (seed, step)); the kernel leaves step + 1 in ``state``.  thr: device int32 [R] holding the uint32 thresholds."""
    require_cuda(state, thr, scale)
    R = thr.numel()
    table = torch.empty(R, B, dtype=torch.float32, device=state.device)
    check(lib().mv_drop_path_draw(_p(state), _p(thr), _p(scale), _p(table), R, B, _s()), "drop_path_draw", R=R, B=B)
    return table


def _row_scale_dims(t, c):
    B = c.numel()
    if t.shape[0] != B or not t.is_contiguous() or c.dtype != torch.float32 or not c.is_contiguous():
        raise ValueError(f"per-sample scale: expected a contiguous [{B}, ...] tensor and a contiguous fp32 [{B}] scale, got "
                         f"{tuple(t.shape)} and {tuple(c.shape)} {c.dtype}")
    return B, t.numel() // B if B else 0


def drop_path_add(x, f, c):
    """In place on f (fp32, shaped like x): f[b] = x[b] + c[b] * f[b], exactly x[b] where c[b] == 0.  Returns f."""
    require_cuda(x, f, c)
    if x.dtype != torch.float32 or f.dtype != torch.float32 or x.shape != f.shape or not x.is_contiguous():
        raise ValueError("drop_path_add: x and f are contiguous fp32 tensors of one shape")
    B, per = _row_scale_dims(f, c)
    check(lib().mv_drop_path_add(_p(x), _p(f), _p(c), B, per, _s()), "drop_path_add", B=B, per_sample=per)
    return f


def row_scale(x, c, out_dtype=None, out=None):
    """c[b] * x[b] (fp32 product, rounded once) as a new tensor of ``out_dtype`` (default: x's), or into ``out`` (contiguous, x's
    shape, not x itself); fp32 or bf16 either side."""
    require_cuda(x, c, out)
    out_dtype = (x.dtype if out_dtype is None else out_dtype) if out is None else out.dtype
    B, per = _row_scale_dims(x, c)
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    elif out.shape != x.shape or not out.is_contiguous() or out.data_ptr() == x.data_ptr():
        raise ValueError("row_scale: out is a contiguous tensor of x's shape, distinct from x")
    check(lib().mv_row_scale(_p(x), _DT[x.dtype], _p(out), _DT[out_dtype], _p(c), B, per, _s()), "row_scale", B=B, per_sample=per)
    return out


# ------------------------------------------------------------------------------------------------------------
# Random Erasing (timm's RandomErasing restated): boxes drawn and filled on the device
# ------------------------------------------------------------------------------------------------------------
RANDOM_ERASE_MODES = {"const": 0, "rand": 1, "pixel": 2}
RANDOM_ERASE_MAX_COUNT = 8            # erases per sample (csrc/random_erase.hip)
RANDOM_ERASE_WAVES = 4                # per workgroup of mv_random_erase_apply: one (channel, box row) each per pass
RANDOM_ERASE_ROWS_PER_BLOCK = 32      # its grid has ceil(Ch * H / this) row bands per (sample, erase) slot ...
RANDOM_ERASE_MAX_BANDS = 32           # ... and never more than this many: the Ch * h rows of a box go round bands * waves workers


def random_erase_draw(state, B, H, W, *, thr, min_area, max_area, log_ratio, min_count, max_count):
    """One launch (mv_random_erase_draw): fresh ``boxes`` int32 [B, max_count, 4] = (top, left, h, w), zeros where nothing is
    erased, and ``used`` int64 [2] = the (seed, step) of this draw, from the Philox stream of ``state`` (device int64[2] = (seed,
    step)); the kernel leaves step + 1 in ``state``.  thr = int(probability * 2**32); log_ratio = (log min_aspect, log max_aspect).
    -> (boxes, used)"""
    require_cuda(state)
    boxes = torch.empty(B, max_count, 4, dtype=torch.int32, device=state.device)
    used = torch.empty(2, dtype=torch.int64, device=state.device)
    area_ratio = (ctypes.c_double * 4)(float(min_area), float(max_area), float(log_ratio[0]), float(log_ratio[1]))   # read by the call
    check(lib().mv_random_erase_draw(_p(state), _p(boxes), _p(used), B, H, W, int(thr), ctypes.addressof(area_ratio), int(min_count),
                                     int(max_count), _s()),
          "random_erase_draw", B=B, H=H, W=W, thr=thr, min_area=min_area, max_area=max_area, log_ratio=tuple(log_ratio),
          min_count=min_count, max_count=max_count)
    return boxes, used


def random_erase_apply(x, boxes, used, mode):
    """Fill the boxes of a dense [B, Ch, H, W] fp32 / bf16 batch IN PLACE (mv_random_erase_apply; write-only): ``mode`` "const"
    (+0.0), "rand" (one normal per sample, box and channel) or "pixel" (one normal per element).  boxes: int32 [B, max_count, 4]
    and used: int64 [2], as ``random_erase_draw`` returns them.  -> x"""
    require_cuda(x, boxes, used)
    if mode not in RANDOM_ERASE_MODES:
        raise ValueError(f"random_erase_apply: mode is one of {sorted(RANDOM_ERASE_MODES)}, got {mode!r}")
    if x.dim() != 4 or not x.is_contiguous() or x.dtype not in _DT:
        raise RuntimeError("random_erase_apply: a contiguous [B, Ch, H, W] fp32 or bf16 batch expected "
                           f"(got {tuple(x.shape)}, {x.dtype}, contiguous={x.is_contiguous()})")
    B, Ch, H, W = x.shape
    if (boxes.dtype != torch.int32 or boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or not boxes.is_contiguous()
            or used.dtype != torch.int64 or used.numel() != 2 or not used.is_contiguous()):
        raise ValueError(f"random_erase_apply: boxes is a contiguous int32 [{B}, max_count, 4] and used a contiguous int64 [2], got "
                         f"{tuple(boxes.shape)} {boxes.dtype} and {tuple(used.shape)} {used.dtype}")
    check(lib().mv_random_erase_apply(_p(x), _DT[x.dtype], _p(boxes), _p(used), B, Ch, H, W, boxes.shape[1],
                                      RANDOM_ERASE_MODES[mode], _s()),
          "random_erase_apply", B=B, Ch=Ch, H=H, W=W, max_count=boxes.shape[1], mode=mode)
    return x


# ------------------------------------------------------------------------------------------------------------
# RandAugment (timm's increasing op set restated): the worker draws, these two launches per slot compute the pixels
# ------------------------------------------------------------------------------------------------------------
def _randaug_check(name, src, ra_op, slot, ra_par=None):
    require_cuda(src, ra_op, ra_par)
    if src.dtype != torch.uint8 or src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous():
        raise ValueError(f"{name}: a contiguous uint8 [B, H, W, 3] batch expected, got {tuple(src.shape)} {src.dtype}")
    B = src.shape[0]
    if ra_op.dtype != torch.int32 or ra_op.dim() != 2 or ra_op.shape[0] != B or not ra_op.is_contiguous():
        raise ValueError(f"{name}: ra_op is a contiguous int32 [{B}, num_ops], got {tuple(ra_op.shape)} {ra_op.dtype}")
    num_ops = ra_op.shape[1]
    if not 0 <= slot < num_ops:
        raise ValueError(f"{name}: slot {slot} outside [0, {num_ops})")
    if ra_par is not None and (ra_par.dtype != torch.float64 or tuple(ra_par.shape) != (B, num_ops, 8) or not ra_par.is_contiguous()):
        raise ValueError(f"{name}: ra_par is a contiguous float64 [{B}, {num_ops}, 8], got {tuple(ra_par.shape)} {ra_par.dtype}")
    return B, src.shape[1], src.shape[2], num_ops


def randaug_stats(src, ra_op, slot, tables=None, mean=None):
    """One launch (mv_randaug_stats) for slot ``slot`` of a uint8 [B, H, W, 3] batch: the AutoContrast / Equalize lookup tables
    (uint8 [B, 3, 256]) and the Contrast means (int32 [B]) of the samples whose op in this slot needs them; other samples' rows
    are not written.  -> (tables, mean)"""
    B, H, W, num_ops = _randaug_check("randaug_stats", src, ra_op, slot)
    if tables is None:
        tables = torch.empty(B, 3, 256, dtype=torch.uint8, device=src.device)
    if mean is None:
        mean = torch.empty(B, dtype=torch.int32, device=src.device)
    if (tables.dtype != torch.uint8 or tuple(tables.shape) != (B, 3, 256) or not tables.is_contiguous() or mean.dtype != torch.int32
            or tuple(mean.shape) != (B,) or not mean.is_contiguous()):
        raise ValueError(f"randaug_stats: tables is a contiguous uint8 [{B}, 3, 256] and mean a contiguous int32 [{B}]")
    require_cuda(tables, mean)
    check(lib().mv_randaug_stats(_p(src), _p(ra_op), num_ops, slot, _p(tables), _p(mean), B, H, W, _s()),
          "randaug_stats", B=B, H=H, W=W, num_ops=num_ops, slot=slot)
    return tables, mean


def randaug_apply(src, ra_op, ra_par, slot, tables, mean, fill=(128, 128, 128), out=None):
    """One launch (mv_randaug_apply): slot ``slot`` of every sample, out of place.  ra_op int32 [B, num_ops] (0 = copy, 1..15 =
    index + 1 in ``datasets.transforms.RANDAUG_OPS``), ra_par float64 [B, num_ops, 8], tables / mean from ``randaug_stats`` of the same slot and ``src``.
    -> uint8 [B, H, W, 3], every byte written"""
    B, H, W, num_ops = _randaug_check("randaug_apply", src, ra_op, slot, ra_par)
    if out is None:
        out = torch.empty_like(src)
    if out.dtype != torch.uint8 or out.shape != src.shape or not out.is_contiguous() or out.data_ptr() == src.data_ptr():
        raise ValueError("randaug_apply: out is a contiguous uint8 tensor of src's shape and not src itself")
    if (tables.dtype != torch.uint8 or tuple(tables.shape) != (B, 3, 256) or not tables.is_contiguous() or mean.dtype != torch.int32
            or tuple(mean.shape) != (B,) or not mean.is_contiguous()):
        raise ValueError(f"randaug_apply: tables is a contiguous uint8 [{B}, 3, 256] and mean a contiguous int32 [{B}]")
    require_cuda(tables, mean, out)
    check(lib().mv_randaug_apply(_p(src), _p(out), _p(ra_op), _p(ra_par), num_ops, slot, _p(tables), _p(mean), int(fill[0]),
                                 int(fill[1]), int(fill[2]), B, H, W, _s()),
          "randaug_apply", B=B, H=H, W=W, num_ops=num_ops, slot=slot, fill=tuple(fill))
    return out
