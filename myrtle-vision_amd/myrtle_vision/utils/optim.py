"""Optimizer and LR schedule of the reference training loop on the HIP AdamW kernel.

The reference builds them with ``timm.optim.create_optimizer`` / ``timm.scheduler.create_scheduler``
(classification/train.py:161-166) from the namespace ``get_optimizer_args`` fills (utils/models.py:84-110).
timm==0.5.4 is not available offline and the reference has no tests for it: the semantics below are a
restatement (PARITY UNPINNED, see oracle/optim_oracle.py for the CPU restatement the tests compare with):

* ``create_optimizer`` with opt="adamw": ``torch.optim.AdamW`` over two groups -- parameters with
  ``ndim <= 1`` or a name ending in ``.bias`` get weight_decay 0, the rest ``weight_decay``; ViT defines no
  ``no_weight_decay()`` so pos_embedding / cls_token ARE decayed.
* ``create_scheduler`` with sched="cosine": ``CosineLRScheduler(t_initial=epochs, lr_min=min_lr,
  warmup_lr_init=warmup_lr, warmup_t=warmup_epochs, cycle_limit=1, t_in_epochs=True)``, stepped with the
  0-based epoch at epoch END (classification/train.py:287).

MI355X-native layout: all trainable, *used* parameters live in ONE flat fp32 arena per weight-decay group
(``ParamArena``); ``param.data`` and ``param.grad`` are views into it.  The optimizer step is then one kernel
launch per group over 86 M contiguous elements (HBM-bound: 7 x 4 B per element), ``zero_grad`` is one memset, and
the DDP gradient all-reduce (``utils/ddp.py``) works on contiguous slices of the same buffer with no packing.

An extension beyond the reference: the optional ``train_config`` keys ``layer_decay``, ``no_weight_decay`` and ``model_ema_decay``
(timm's layer-wise learning-rate decay and ``no_weight_decay`` list, a model EMA) select ``TableAdamW`` below -- a learning-rate
scale and a weight decay per TENSOR and a weight EMA, stepped with ONE launch over the whole arena (``mv_adamw_table``).  Without
the keys ``create_optimizer`` builds the ``AdamW`` described above and none of that code runs.

A second extension: ``"optimizer": "sgd"`` / ``"momentum"`` / ``"lamb"`` (timm's names; every reference config says ``"adamw"``) build
``TableSGD`` and ``TableLamb`` on the same frame and the same work list (``csrc/optim_family.hip``).  ``TableSGD`` is
``torch.optim.SGD`` with dampening 0, Nesterov for ``"sgd"`` and plain momentum for ``"momentum"`` as in timm, and is held to torch by
the tests.  ``TableLamb`` restates timm's ``Lamb`` with bias correction on, ``always_adapt=False`` and ``trust_clip=False`` (PARITY
UNPINNED, as above: timm is not available offline; the formulas in ``TableLamb``'s docstring are the definition, the tests hold the
kernel to their fp64 evaluation).
"""
import contextlib
import math
from typing import Iterable, List, Tuple

import torch

from myrtle_vision.hip import ops


class ParamArena:
    """Flat fp32 storage for parameters and their gradients, split into (decay, no_decay) regions."""

    def __init__(self, named_params: Iterable[Tuple[str, torch.nn.Parameter]], skip=()):
        every = [(n, p) for n, p in named_params if p.requires_grad]
        named = [(n, p) for n, p in every if n not in set(skip)]
        if not named:
            raise ValueError("no trainable parameters")
        # parameter order of the torch.optim.AdamW the reference builds through timm (add_weight_decay: the no-decay group
        # first, then the decayed one, each in named_parameters order, the never-used detection parameters included):
        # the integer keys of the optimizer part of a reference checkpoint index into this list
        nd = lambda n, p: p.ndim <= 1 or n.endswith(".bias")
        self.torch_groups = [[n for n, p in every if nd(n, p)], [n for n, p in every if not nd(n, p)]]
        dev = named[0][1].device
        decay, no_decay = [(n, p) for n, p in named if not nd(n, p)], [(n, p) for n, p in named if nd(n, p)]
        self.names: List[str] = [n for n, _ in decay + no_decay]
        self.params: List[torch.nn.Parameter] = [p for _, p in decay + no_decay]
        # each tensor starts on a 32-byte boundary: kernels can use 16-byte vector access on any slice of the fp32 arena AND
        # of its bf16 staging copy (the half-width gradient exchange casts bucket slices, utils/ddp.py)
        offs, total = [], 0
        for _, p in decay + no_decay:
            offs.append(total)
            total += (p.numel() + 7) & ~7
        self.n_decay = offs[len(decay)] if no_decay and decay else (total if decay else 0)
        self.offsets, self.total = offs, total
        self.flat_param = torch.zeros(total, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(total, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                n = p.numel()
                self.flat_param[o:o + n].copy_(p.detach().reshape(-1).float())
                p.data = self.flat_param[o:o + n].view(p.shape)
                p.grad = None
                ops.register_grad_slot(p, self.flat_grad[o:o + n])      # backward kernels write d/dp here directly
        # any torch-side in-place write to the flat buffer (loading into the arena, an EMA, a custom collective) moves the
        # weight caches' epoch by itself; raw-pointer writes (the AdamW kernel) announce themselves through bump_versions()
        ops.register_arena(self.flat_param)

    def slot(self, j):
        o = self.offsets[j]
        return self.flat_grad[o:o + self.params[j].numel()]

    def zero_grad(self):
        """``set_to_none`` semantics: with no gradient attached, the backward kernels write each parameter's gradient
        straight into its arena slot and autograd adopts that view (``ops.grad_out``) -- no zero-fill, no adds."""
        for p in self.params:
            p.grad = None

    def sync_grad(self, j):
        """Make slot j hold parameter j's gradient: a no-op on the fast path (the gradient already IS the slot);
        copies a gradient autograd materialised elsewhere; zero-fills the slot of a parameter that received none."""
        p, slot = self.params[j], self.slot(j)
        g = p.grad
        if g is None:
            slot.zero_()
        elif g.data_ptr() != slot.data_ptr():
            slot.copy_(g.detach().reshape(-1))
            p.grad = slot.view(p.shape)

    def sync_grads(self):
        for j in range(len(self.params)):
            self.sync_grad(j)

    def bump_versions(self):
        """The AdamW kernel writes through raw pointers: tell autograd / the bf16 weight cache the data changed."""
        for p in self.params:
            torch.autograd.graph.increment_version(p)
        ops.invalidate_weight_caches(self.flat_param)


class AdamW:
    """torch.optim.AdamW semantics on the fused HIP kernel over a ``ParamArena`` (one launch per decay group)."""
    ema, ema_loaded = None, False        # no weight EMA here (``TableAdamW`` may keep one): the loops ask every optimizer
    kind = "adamw"                       # what a checkpoint of this optimizer is; "adamw" is not written (the reference's format)
    state_names = ("exp_avg", "exp_avg_sq")      # the per-parameter state of a checkpoint: attributes shaped like the arena
    step_in_state = True                 # torch.optim.AdamW keeps a ``step`` per parameter; else the checkpoint has one ``step_count``
    optional_state = {}                  # state name -> the error when a checkpoint carries it and this optimizer keeps no such array;
                                         # an entry may lack (or hold None for) these names only

    def __init__(self, arena: ParamArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self.arena = arena
        self.defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)
        nd = arena.n_decay
        self.param_groups = [
            dict(lr=lr, initial_lr=lr, weight_decay=weight_decay, range=(0, nd), name="decay"),
            dict(lr=lr, initial_lr=lr, weight_decay=0.0, range=(nd, arena.total), name="no_decay"),
        ]
        self._init_state()
        self.step_count = 0
        self.grad_scale = 1.0            # e.g. 1/world_size after a SUM all-reduce
        self.max_grad_norm = None        # train_config.clip_grad: clip_grad_norm_ folded into the step (train.py:265-270)
        self.last_grad_norm = None       # device tensor [total_norm, clip coefficient] of the last clipped step
        self._hyper = None               # use_device_scalars(): per-group fp32 [3] (lr, bias_corr1, bias_corr2) on the device

    def _init_state(self):
        """The state arrays, shaped like the arena (a subclass with other state allocates its own instead)."""
        self.exp_avg = torch.zeros_like(self.arena.flat_param)
        self.exp_avg_sq = torch.zeros_like(self.arena.flat_param)

    def _bias_corrections(self):
        """(1 - beta1^t, 1 - beta2^t) at the current step count."""
        b1, b2 = self.defaults["betas"]
        return 1.0 - b1 ** self.step_count, 1.0 - b2 ** self.step_count

    def _clip_norm(self):
        """The norm ``step()`` clips the gradient to, or None: ``train_config.clip_grad``."""
        return self.max_grad_norm

    def _check_kind(self, sd):
        kind = sd.get("kind", "adamw")
        if kind != self.kind:
            raise ValueError(f"optimizer checkpoint was written by a {kind!r} optimizer, this one is {self.kind!r}")

    # -- per-step scalars on the device (HIP-graph capture: utils/graph.py) ---------------------------------------------
    def use_device_scalars(self, ring: int = 32):
        """From now on the kernels read lr and the two bias corrections from device memory instead of launch arguments, so a
        captured ``step()`` stays valid while the schedule and the step count advance.  ``advance()`` (called by ``step()``
        itself outside a capture, by the graph's replayer otherwise) bumps the step count and sends the new values: pinned
        staging slots in a ring, each guarded by an event, so the host may run many steps ahead of the device."""
        dev = self.arena.flat_param.device
        self._hyper = {g["name"]: torch.zeros(3, dtype=torch.float32, device=dev) for g in self.param_groups}
        self._stage = [torch.zeros(len(self.param_groups), 3, dtype=torch.float32).pin_memory() for _ in range(ring)]
        self._stage_done = [None] * ring
        self._stage_i = 0

    def advance(self):
        """step_count += 1 and (lr, 1 - beta1^t, 1 - beta2^t) of every group -> the device, on the current stream."""
        self.step_count += 1
        bc1, bc2 = self._bias_corrections()
        i = self._stage_i
        self._stage_i = (i + 1) % len(self._stage)
        if self._stage_done[i] is not None:
            self._stage_done[i].synchronize()           # the copy that last read this slot has run (normally long ago)
        host = self._stage[i]
        for r, g in enumerate(self.param_groups):
            host[r, 0], host[r, 1], host[r, 2] = g["lr"], bc1, bc2
        for r, g in enumerate(self.param_groups):
            self._hyper[g["name"]].copy_(host[r], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._stage_done[i] = ev

    def zero_grad(self, set_to_none: bool = False):
        self.arena.zero_grad()

    @torch.no_grad()
    def clip_accumulated(self):
        """``clip_grad_norm_`` on the running accumulated gradient BETWEEN the micro-batches of an accumulation window
        (classification/train.py:265-270 runs it after every backward): the arena becomes grad_scale * coefficient * itself, in
        place -- the pending 1/world of a SUM all-reduce is applied here, so the next micro-batch adds to the averaged, clipped
        gradient exactly as the reference's does.  No host synchronisation (norm and coefficient stay on the device)."""
        if self.max_grad_norm is None:
            return
        self.arena.sync_grads()
        a = self.arena
        self.last_grad_norm = ops.grad_norm_clip(a.flat_grad, self.max_grad_norm, self.grad_scale)
        a.flat_grad.mul_(self.last_grad_norm[1] * self.grad_scale)

    @torch.no_grad()
    def step(self):
        """The frame of every step: gradients into their slots, the count, the optional clip reduction, ``_launch``, versions."""
        self.arena.sync_grads()
        if self._hyper is None:
            self.step_count += 1
        elif not torch.cuda.is_current_stream_capturing():
            self.advance()                # inside a capture the replayer advances (utils/graph.py)
        a = self.arena
        coef, max_norm = None, self._clip_norm()
        if max_norm is not None:
            # torch.nn.utils.clip_grad_norm_ over every parameter that has a gradient = the whole arena (alignment gaps
            # hold zeros): one norm reduction, and the coefficient rides into the AdamW kernel as a device scalar
            self.last_grad_norm = ops.grad_norm_clip(a.flat_grad, max_norm, self.grad_scale)
            coef = self.last_grad_norm[1:2]
        self._launch(coef)
        a.bump_versions()

    def _shared_kw(self, coef, g, ema=False):
        """The keywords every launch of group ``g`` is handed besides its own arithmetic: the gradient scale, the clip coefficient, the
        group's scalars on the device (``use_device_scalars``) and, for a one-launch table step (``ema``), the weight EMA."""
        kw = dict(grad_scale=self.grad_scale, clip_coef=coef, hyper=None if self._hyper is None else self._hyper[g["name"]])
        if ema:
            kw.update(ema=self.ema, ema_decay=self.ema_decay if self.ema is not None else 0.0)
        return kw

    def _launch(self, coef):
        """One launch per non-empty group, the decay group first."""
        a, (b1, b2) = self.arena, self.defaults["betas"]
        for g in self.param_groups:
            lo, hi = g["range"]
            if hi > lo:
                ops.adamw_step(a.flat_param[lo:hi], a.flat_grad[lo:hi], self.exp_avg[lo:hi], self.exp_avg_sq[lo:hi],
                               lr=g["lr"], beta1=b1, beta2=b2, eps=self.defaults["eps"],
                               weight_decay=g["weight_decay"], step=self.step_count, **self._shared_kw(coef, g))

    # checkpoint format = torch.optim.AdamW.state_dict() of the optimizer the reference builds (classification/train.py:
    # 161-166, utils/models.py:113-126): ``state`` keyed by the parameter's index in timm's group order with a per-parameter
    # ``step``, ``param_groups`` = [no_decay, decay] carrying those indices.  ``param_names`` (index -> name) is an extra
    # key torch ignores.  Parameters that never received a gradient (the detection tokens) have no state, as in torch.  A subclass
    # says what differs: ``state_names``, ``optional_state``, ``step_in_state``, ``_group_fields`` and its ``kind``, written whenever it is not "adamw".
    def _torch_index(self):
        names = self.arena.torch_groups[0] + self.arena.torch_groups[1]
        return {n: i for i, n in enumerate(names)}, names

    def _group_fields(self):
        """What a torch param group of this optimizer carries besides lr, weight_decay, initial_lr and params."""
        return {"betas": self.defaults["betas"], "eps": self.defaults["eps"], "amsgrad": False, "maximize": False}

    def state_dict(self):
        a = self.arena
        index, names = self._torch_index()
        arrays = {k: getattr(self, k) for k in self.state_names if getattr(self, k) is not None}
        state = {}
        if self.step_count > 0 and arrays:
            for n, p, o in zip(a.names, a.params, a.offsets):
                state[index[n]] = {"step": self.step_count} if self.step_in_state else {}
                state[index[n]].update({k: arr[o:o + p.numel()].view(p.shape).clone() for k, arr in arrays.items()})
        by_name = {g["name"]: g for g in self.param_groups}
        groups, first = [], 0
        for gname, members in zip(("no_decay", "decay"), a.torch_groups):
            g = by_name[gname]
            groups.append({"lr": g["lr"], **self._group_fields(), "weight_decay": g["weight_decay"], "initial_lr": g["initial_lr"],
                           "params": list(range(first, first + len(members)))})
            first += len(members)
        sd = {"state": state, "param_groups": groups, "param_names": names}
        if self.kind != "adamw":
            sd["kind"] = self.kind
        if not self.step_in_state:
            sd["step_count"] = self.step_count
        return sd

    def load_state_dict(self, sd):
        self._check_kind(sd)
        a = self.arena
        index, names = self._torch_index()
        st = sd["state"]
        if "param_names" in sd and list(sd["param_names"]) != names:
            raise ValueError("optimizer checkpoint was written for a different parameter list")
        legacy = any(isinstance(k, str) for k in st)            # round-1 layout: keyed by name, one top-level step
        steps = set()
        for n, p, o in zip(a.names, a.params, a.offsets):
            ent = st.get(n) if legacy else st.get(index[n])
            if ent is None:
                continue
            for k in self.state_names:
                if k in self.optional_state and ent.get(k) is None:
                    continue
                if getattr(self, k) is None:
                    raise ValueError(self.optional_state[k])
                if tuple(ent[k].shape) != tuple(p.shape):
                    raise ValueError(f"optimizer state of {n}: shape {tuple(ent[k].shape)} != {tuple(p.shape)}")
                getattr(self, k)[o:o + p.numel()].copy_(ent[k].reshape(-1))
            if "step" in ent:
                steps.add(int(ent["step"]))
        if legacy:
            self.step_count = int(sd["step"])
        elif not self.step_in_state:
            self.step_count = int(sd.get("step_count", 0))
        else:
            if len(steps) > 1:
                raise ValueError(f"per-parameter steps differ ({sorted(steps)}): one fused step counter cannot hold them")
            self.step_count = steps.pop() if steps else 0
        by_name = {g["name"]: g for g in self.param_groups}
        order = ("decay", "no_decay") if legacy else ("no_decay", "decay")
        for gname, s in zip(order, sd["param_groups"]):
            by_name[gname].update({k: v for k, v in s.items() if k in ("lr", "initial_lr", "weight_decay")})


# ---- layer-wise learning-rate decay, weight-decay exemptions and a weight EMA: ONE launch over the arena (mv_adamw_table) ----------
_LAYER0 = ("pos_embedding", "cls_token", "det_tokens", "pos_embedding_det")
ITEM_MAX = 4096                          # elements per work item of mv_adamw_table (include/myrtle_vision_hip.h)


def vit_depth(names) -> int:
    """Number of transformer blocks among parameter names (``transformer.layers.{i}.*``)."""
    blocks = [int(n.split(".")[2]) for n in names if n.startswith("transformer.layers.")]
    return max(blocks) + 1 if blocks else 0


def layer_ids(names, depth=None) -> List[int]:
    """timm's ViT grouping for layer-wise learning-rate decay: 0 for the embeddings (``pos_embedding``, ``cls_token``,
    ``patch_to_embedding.*``, ``det_tokens``, ``pos_embedding_det``), i + 1 for ``transformer.layers.{i}.*``, depth + 1 for
    everything else (the decoder of any task)."""
    names = list(names)
    depth = vit_depth(names) if depth is None else depth
    ids = []
    for n in names:
        if n in _LAYER0 or n.startswith("patch_to_embedding."):
            ids.append(0)
        elif n.startswith("transformer.layers."):
            ids.append(int(n.split(".")[2]) + 1)
        else:
            ids.append(depth + 1)
    return ids


def layer_scales(names, layer_decay, depth=None) -> List[float]:
    """``lr_scale = layer_decay ** (depth + 1 - layer_id)``: 1 for the head, ``layer_decay ** (depth + 1)`` for the embeddings."""
    names = list(names)
    depth = vit_depth(names) if depth is None else depth
    return [float(layer_decay) ** (depth + 1 - i) for i in layer_ids(names, depth)]


def build_items(offsets, sizes, pairs):
    """Cut tensors into the work items of ``mv_adamw_table``.  ``offsets`` / ``sizes``: each tensor's arena offset (a multiple of 8)
    and element count; ``pairs``: its ``(lr_scale, weight_decay)``.  -> (item offsets, item lengths, item segments, segments):
    three lists of one length and the list of distinct pairs in order of first use.  An item never crosses a tensor, holds at most
    ``ITEM_MAX`` elements and starts at its tensor's offset plus a multiple of ``ITEM_MAX``; the gaps between tensors are in no item."""
    segments, index = [], {}
    off, length, seg = [], [], []
    for o, n, pair in zip(offsets, sizes, pairs):
        pair = (float(pair[0]), float(pair[1]))
        s = index.setdefault(pair, len(segments))
        if s == len(segments):
            segments.append(pair)
        for k in range(0, n, ITEM_MAX):
            off.append(o + k)
            length.append(min(ITEM_MAX, n - k))
            seg.append(s)
    return off, length, seg, segments


def build_item_tensors(sizes):
    """Which items of ``build_items`` form a tensor (what LAMB's per-tensor norms need) -> (the tensor index of every item, every
    tensor's first item, every tensor's item count).  Tensor t has ``ceil(sizes[t] / ITEM_MAX)`` consecutive items."""
    item_tensor, first, count = [], [], []
    for t, n in enumerate(sizes):
        k = (n + ITEM_MAX - 1) // ITEM_MAX
        first.append(len(item_tensor))
        count.append(k)
        item_tensor.extend([t] * k)
    return item_tensor, first, count


def _check_unit(key, value, hi_closed=True):
    """A float in (0, 1] (``hi_closed``) or (0, 1); the message names ``key``."""
    ok = isinstance(value, (int, float)) and not isinstance(value, bool) and value == value
    ok = ok and 0.0 < value and (value <= 1.0 if hi_closed else value < 1.0)
    if not ok:
        raise ValueError(f"{key} must be a number in (0, 1{']' if hi_closed else ')'}, got {value!r}")
    return float(value)


def check_table_options(names, layer_decay=None, no_weight_decay=None, ema_decay=None, ema_key="ema_decay"):
    """The three optional keys, checked against the parameter names ``names`` -> (layer_decay, no_weight_decay as a tuple, ema_decay).
    ``ema_key``: what the caller's user calls the EMA decay (``model_ema_decay`` in a train_config); each message names its key."""
    if layer_decay is not None:
        layer_decay = _check_unit("layer_decay", layer_decay)
    if ema_decay is not None:
        ema_decay = _check_unit(ema_key, ema_decay, hi_closed=False)
    if no_weight_decay is not None:
        if not isinstance(no_weight_decay, (list, tuple)) or not all(isinstance(n, str) for n in no_weight_decay):
            raise ValueError(f"no_weight_decay must be a list of parameter names, got {no_weight_decay!r}")
        for n in no_weight_decay:
            if n not in names:
                raise ValueError(f"no_weight_decay names {n!r}, which is not a parameter of the model")
    return layer_decay, tuple(no_weight_decay or ()), ema_decay


class TableAdamW(AdamW):
    """``AdamW`` with a learning-rate scale and a weight decay PER TENSOR and an optional weight EMA, stepped with ONE
    ``mv_adamw_table`` launch over the whole arena (an extension; the reference has none of the three).

    * ``layer_decay``: timm's layer-wise learning-rate decay (``layer_scales``); the effective rate of a tensor is the scheduled
      base rate times its scale, through warm-up and down to ``min_lr``, as timm applies ``lr_scale``.
    * ``no_weight_decay``: exact parameter names whose weight decay becomes 0 (the arena's layout does not change).
    * ``ema_decay``: ``ema = d * ema + (1 - d) * p`` after every step, in the same pass; ``ema_weights()`` evaluates on it.

    ``param_groups`` stays the two reference groups carrying the scheduled BASE rate, so ``CosineLRScheduler`` works unchanged; the
    two must carry one rate."""

    def __init__(self, arena: ParamArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, layer_decay=None,
                 no_weight_decay=(), ema_decay=None):
        super().__init__(arena, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        known = set(arena.names) | set(arena.torch_groups[0]) | set(arena.torch_groups[1])      # the ones the arena leaves out too
        self.layer_decay, self.no_weight_decay, self.ema_decay = check_table_options(known, layer_decay, no_weight_decay, ema_decay)
        self.lr_scales = layer_scales(arena.names, self.layer_decay) if self.layer_decay is not None else [1.0] * len(arena.names)
        self._tables_wd = None
        self._refresh_tables()
        self._in_ema = False
        if self.ema_decay is not None:
            self.ema = torch.zeros_like(arena.flat_param)
            self.reset_ema()

    def tensor_weight_decays(self) -> List[float]:
        """Each arena tensor's weight decay: its group's, or 0 for a ``no_weight_decay`` name."""
        a, exempt = self.arena, set(self.no_weight_decay)
        by_name = {g["name"]: g["weight_decay"] for g in self.param_groups}
        return [0.0 if n in exempt else float(by_name["decay" if o < a.n_decay else "no_decay"])
                for n, o in zip(a.names, a.offsets)]

    def _refresh_tables(self):
        """(Re)build the device work list and segment tables; they change only when a group's weight decay does (a loaded checkpoint)."""
        wd = tuple(g["weight_decay"] for g in self.param_groups)
        if wd == self._tables_wd:
            return
        a = self.arena
        dev = a.flat_param.device
        off, length, seg, segments = build_items(a.offsets, [p.numel() for p in a.params],
                                                 list(zip(self.lr_scales, self.tensor_weight_decays())))
        self.items = (torch.tensor(off, dtype=torch.int64, device=dev), torch.tensor(length, dtype=torch.int32, device=dev),
                      torch.tensor(seg, dtype=torch.int32, device=dev))
        self.segments = segments
        self.seg_lr_scale = torch.tensor([s for s, _ in segments], dtype=torch.float32, device=dev)
        self.seg_wd = torch.tensor([w for _, w in segments], dtype=torch.float32, device=dev)
        self._tables_wd = wd

    @torch.no_grad()
    def step(self):
        if self._in_ema:
            raise RuntimeError("step() inside ema_weights(): the parameters hold the EMA, not the trained weights")
        lr = self.param_groups[0]["lr"]
        if any(g["lr"] != lr for g in self.param_groups):
            raise ValueError(f"the two param_groups carry different learning rates ({[g['lr'] for g in self.param_groups]}): the one "
                             "launch steps at ONE scheduled rate times each tensor's scale")
        self._refresh_tables()
        super().step()

    def _launch(self, coef):
        """ONE launch over the whole arena, at the first group's (= the one) scheduled rate."""
        a, (b1, b2), g = self.arena, self.defaults["betas"], self.param_groups[0]
        ops.adamw_table_step(a.flat_param, a.flat_grad, self.exp_avg, self.exp_avg_sq, self.items, self.seg_lr_scale, self.seg_wd,
                             lr=g["lr"], beta1=b1, beta2=b2, eps=self.defaults["eps"], step=self.step_count,
                             **self._shared_kw(coef, g, ema=True))

    # -- the weight EMA -------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset_ema(self):
        """EMA <- the current weights (a fresh run, or after loading weights that carried no EMA)."""
        if self.ema is None:
            raise RuntimeError("reset_ema(): this optimizer was built without ema_decay")
        self.ema.copy_(self.arena.flat_param)

    def _swap_ema(self):
        with torch.no_grad():
            tmp = self.arena.flat_param.clone()
            self.arena.flat_param.copy_(self.ema)
            self.ema.copy_(tmp)
        self.arena.bump_versions()

    @contextlib.contextmanager
    def ema_weights(self):
        """``with optimizer.ema_weights(): validate(model)``: the parameters hold the EMA inside the block and the trained weights
        again after it (the two buffers exchange contents, bit for bit)."""
        if self.ema is None:
            raise RuntimeError("ema_weights(): this optimizer was built without ema_decay")
        if self._in_ema:
            raise RuntimeError("ema_weights() does not nest")
        self._swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self._in_ema = False
            self._swap_ema()

    def ema_state_dict(self, model):
        """The model's state dict (host tensors) with every arena parameter replaced by its EMA: a checkpoint's ``"model_ema"``."""
        if self.ema is None:
            raise RuntimeError("ema_state_dict(): this optimizer was built without ema_decay")
        a = self.arena
        sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
        src = self.arena.flat_param if self._in_ema else self.ema        # inside ema_weights() the buffers are exchanged
        for n, p, o in zip(a.names, a.params, a.offsets):
            if n not in sd:
                raise KeyError(f"parameter {n!r} is not a key of the model's state dict")
            sd[n] = src[o:o + p.numel()].view(p.shape).detach().cpu().clone()
        return sd

    @torch.no_grad()
    def load_ema_state_dict(self, sd):
        if self.ema is None:
            raise RuntimeError("load_ema_state_dict(): this optimizer was built without ema_decay")
        a = self.arena
        for n, p, o in zip(a.names, a.params, a.offsets):
            if n not in sd:
                raise KeyError(f"'model_ema' has no entry {n!r}")
            if tuple(sd[n].shape) != tuple(p.shape):
                raise ValueError(f"'model_ema' entry {n}: shape {tuple(sd[n].shape)} != {tuple(p.shape)}")
            self.ema[o:o + p.numel()].copy_(sd[n].reshape(-1))
        self.ema_loaded = True

    # -- checkpoints: AdamW's format plus two keys torch ignores -----------------------------------------------------------
    def state_dict(self):
        sd = super().state_dict()
        sd["layer_decay"] = self.layer_decay
        sd["no_weight_decay"] = list(self.no_weight_decay)
        return sd

    def load_state_dict(self, sd):
        self._check_kind(sd)
        self._check_recipe(sd)
        super().load_state_dict(sd)
        self._refresh_tables()

    def _check_recipe(self, sd):
        if sd.get("layer_decay") != self.layer_decay:
            raise ValueError(f"optimizer checkpoint has layer_decay={sd.get('layer_decay')!r}, this optimizer {self.layer_decay!r}")
        if sorted(sd.get("no_weight_decay", ())) != sorted(self.no_weight_decay):
            raise ValueError(f"optimizer checkpoint has no_weight_decay={list(sd.get('no_weight_decay', ()))!r}, this optimizer "
                             f"{list(self.no_weight_decay)!r}")


class TableSGD(TableAdamW):
    """``torch.optim.SGD`` (dampening 0) on ``TableAdamW``'s frame -- the step, the clip reduction, the device scalars, the EMA,
    ``layer_decay`` and ``no_weight_decay`` are that class's -- stepped with ONE ``mv_sgd_table`` launch over the whole arena:

        d = g + wd * p;  buf = momentum * buf + d;  d = nesterov ? d + momentum * buf : buf;  p -= lr * lr_scale * d

    One state array, ``momentum_buffer``; with ``momentum == 0`` there is none and the kernel reads and writes no buffer.  A
    checkpoint has the layout of the ``torch.optim.SGD`` timm would build (per-parameter ``momentum_buffer``, the two param groups)
    plus ``kind``, ``step_count`` and ``TableAdamW``'s keys, which torch ignores."""
    kind, state_names, step_in_state = "sgd", ("momentum_buffer",), False
    optional_state = {"momentum_buffer": "optimizer checkpoint carries momentum buffers, this optimizer has momentum 0"}

    def __init__(self, arena: ParamArena, lr=1e-3, momentum=0.9, nesterov=False, weight_decay=0.0, layer_decay=None,
                 no_weight_decay=(), ema_decay=None):
        self.momentum, self.nesterov = check_momentum(momentum, nesterov), bool(nesterov)
        super().__init__(arena, lr=lr, weight_decay=weight_decay, layer_decay=layer_decay, no_weight_decay=no_weight_decay,
                         ema_decay=ema_decay)
        self.defaults = dict(lr=lr, momentum=self.momentum, nesterov=self.nesterov, weight_decay=weight_decay)

    def _init_state(self):
        self.momentum_buffer = torch.zeros_like(self.arena.flat_param) if self.momentum != 0 else None

    def _bias_corrections(self):
        return 1.0, 1.0                  # SGD has none; the kernel reads the rate only

    def _group_fields(self):
        return {"momentum": self.momentum, "dampening": 0, "nesterov": self.nesterov, "maximize": False}

    def _launch(self, coef):
        a, g = self.arena, self.param_groups[0]
        ops.sgd_table_step(a.flat_param, a.flat_grad, self.momentum_buffer, self.items, self.seg_lr_scale, self.seg_wd, lr=g["lr"],
                           momentum=self.momentum, nesterov=self.nesterov, **self._shared_kw(coef, g, ema=True))


class TableLamb(TableAdamW):
    """LAMB on ``TableAdamW``'s frame, state and checkpoint layout (``exp_avg``, ``exp_avg_sq``, the step count; plus ``kind``),
    stepped with ``mv_lamb_table``: two launches over the whole arena and a per-tensor reduction between them that uses no atomics,
    no memset and no host read.  With ``gr`` the gradient after the clip, ``bc1 = 1 - beta1^t``, ``bc2 = 1 - beta2^t``, per tensor:

        m = beta1 * m + (1 - beta1) * gr;  v = beta2 * v + (1 - beta2) * gr * gr
        u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd * p
        trust = (wd != 0 and ||p|| > 0 and ||u|| > 0) ? ||p|| / ||u|| : 1
        p = p - lr * lr_scale * trust * u

    This is the arithmetic of timm's ``Lamb`` with bias correction on, ``always_adapt=False`` and ``trust_clip=False``, restated:
    timm is not available offline, so the class is NOT pinned by parity to timm (PARITY UNPINNED, as the module docstring says of
    the schedule); the formulas above are the definition and the tests hold the kernel to their fp64 evaluation.

    timm's ``Lamb`` always clips the global gradient norm first (``max_grad_norm=1.0``): here ``lamb_max_grad_norm`` (None switches it
    off), one ``ops.grad_norm_clip`` whose coefficient rides into the first launch.  With ``clip_grad`` (``max_grad_norm``) set as
    well the step clips ONCE, to the smaller of the two: clipping to c and then to 1 is clipping to min(c, 1).  (The coefficient is
    ``min(1, max_norm / (norm + 1e-6))``, ``clip_grad_norm_``'s; timm's own has no 1e-6.)"""
    kind = "lamb"

    def __init__(self, arena: ParamArena, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, lamb_max_grad_norm=1.0,
                 layer_decay=None, no_weight_decay=(), ema_decay=None):
        self.lamb_max_grad_norm = check_lamb_max_grad_norm(lamb_max_grad_norm)
        self.item_tensor = None
        super().__init__(arena, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, layer_decay=layer_decay,
                         no_weight_decay=no_weight_decay, ema_decay=ema_decay)

    def _refresh_tables(self):
        super()._refresh_tables()
        if self.item_tensor is None:     # which items form a tensor, and the partial sums' home: sizes only, built ONCE
            dev = self.arena.flat_param.device
            item_tensor, first, count = build_item_tensors([p.numel() for p in self.arena.params])
            self.item_tensor = torch.tensor(item_tensor, dtype=torch.int32, device=dev)
            self.tensor_range = torch.tensor(list(zip(first, count)), dtype=torch.int32, device=dev).reshape(-1, 2)
            self.workspace = ops.lamb_workspace(len(item_tensor), dev)

    def _clip_norm(self):
        norms = [n for n in (self.max_grad_norm, self.lamb_max_grad_norm) if n is not None]
        return min(norms) if norms else None

    def _launch(self, coef):
        a, (b1, b2), g = self.arena, self.defaults["betas"], self.param_groups[0]
        ops.lamb_table_step(a.flat_param, a.flat_grad, self.exp_avg, self.exp_avg_sq, self.items, self.item_tensor, self.tensor_range,
                            self.seg_lr_scale, self.seg_wd, self.workspace, lr=g["lr"], beta1=b1, beta2=b2, eps=self.defaults["eps"],
                            step=self.step_count, **self._shared_kw(coef, g, ema=True))


def check_momentum(momentum, nesterov):
    """``momentum``: a number in [0, 1), and not 0 with Nesterov (what torch.optim.SGD refuses too)."""
    if not isinstance(momentum, (int, float)) or isinstance(momentum, bool) or not 0.0 <= momentum < 1.0:
        raise ValueError(f"momentum must be a number in [0, 1), got {momentum!r}")
    if nesterov and momentum == 0:
        raise ValueError("\"optimizer\": \"sgd\" is Nesterov momentum (timm's meaning) and needs momentum > 0; \"momentum\" is the "
                         "plain form")
    return float(momentum)


def check_lamb_max_grad_norm(value):
    """``lamb_max_grad_norm``: a positive number, or None (no clip of LAMB's own)."""
    if value is None:
        return None
    if not isinstance(value, (int, float)) or isinstance(value, bool) or not value > 0:
        raise ValueError(f"lamb_max_grad_norm must be a positive number or null, got {value!r}")
    return float(value)


class CosineLRScheduler:
    """timm 0.5.4 ``CosineLRScheduler`` restated for cycle_limit=1, t_in_epochs=True, no noise, warmup_prefix False."""

    def __init__(self, optimizer, t_initial, lr_min=0.0, warmup_t=0, warmup_lr_init=0.0):
        self.optimizer = optimizer
        self.t_initial, self.lr_min, self.warmup_t, self.warmup_lr_init = t_initial, lr_min, warmup_t, warmup_lr_init
        self.base_values = [g["initial_lr"] for g in optimizer.param_groups]
        if warmup_t:
            self.warmup_steps = [(v - warmup_lr_init) / warmup_t for v in self.base_values]
            self._update([warmup_lr_init for _ in self.base_values])   # timm sets warmup_lr_init at construction
        else:
            self.warmup_steps = [1 for _ in self.base_values]

    def _get_lr(self, t):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * s for s in self.warmup_steps]
        if t < self.t_initial:
            return [self.lr_min + 0.5 * (v - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial))
                    for v in self.base_values]
        return [self.lr_min for _ in self.base_values]

    def _update(self, values):
        for g, v in zip(self.optimizer.param_groups, values):
            g["lr"] = v

    def step(self, epoch, metric=None):
        self._update(self._get_lr(epoch))

    def state_dict(self):
        return {k: v for k, v in self.__dict__.items() if k != "optimizer"}

    def load_state_dict(self, sd):
        self.__dict__.update(sd)


OPTIMIZERS = ("adamw", "sgd", "momentum", "lamb")


def create_optimizer(args, model, skip=None):
    """Counterpart of ``timm.optim.create_optimizer(args, model)`` for the options the reference configs use."""
    opt = str(args.opt).lower()
    if opt not in OPTIMIZERS:
        raise NotImplementedError(f"optimizer {args.opt!r}: implemented are {', '.join(repr(o) for o in OPTIMIZERS)} ('adamw' is "
                                  "what every reference train_config uses)")
    if skip is None:
        skip = model.unused_parameter_names() if hasattr(model, "unused_parameter_names") else ()
    # optional train_config keys (an extension): any of them selects the one-launch TableAdamW; without them the object, its
    # two launches and everything else are the reference optimizer's.  Checked before the arena takes over the parameters.
    layer_decay, ema_decay = getattr(args, "layer_decay", None), getattr(args, "model_ema_decay", None)
    no_weight_decay = getattr(args, "no_weight_decay", None)
    check_table_options({n for n, _ in model.named_parameters()}, layer_decay, no_weight_decay, ema_decay, ema_key="model_ema_decay")
    if opt in ("sgd", "momentum"):
        check_momentum(args.momentum, opt == "sgd")
    elif opt == "lamb":
        check_lamb_max_grad_norm(getattr(args, "lamb_max_grad_norm", 1.0))
    arena = ParamArena(model.named_parameters(), skip=skip)
    betas = tuple(args.opt_betas) if getattr(args, "opt_betas", None) else (0.9, 0.999)
    table = dict(layer_decay=layer_decay, no_weight_decay=no_weight_decay or (), ema_decay=ema_decay)
    if opt in ("sgd", "momentum"):       # timm's meanings: "sgd" is Nesterov, "momentum" is not; both take args.momentum
        return TableSGD(arena, lr=args.lr, momentum=args.momentum, nesterov=opt == "sgd", weight_decay=args.weight_decay, **table)
    if opt == "lamb":
        eps = args.opt_eps if getattr(args, "opt_eps", None) is not None else 1e-6
        return TableLamb(arena, lr=args.lr, betas=betas, eps=eps, weight_decay=args.weight_decay,
                         lamb_max_grad_norm=getattr(args, "lamb_max_grad_norm", 1.0), **table)
    eps = args.opt_eps if getattr(args, "opt_eps", None) is not None else 1e-8
    if layer_decay is None and ema_decay is None and no_weight_decay is None:
        return AdamW(arena, lr=args.lr, betas=betas, eps=eps, weight_decay=args.weight_decay)
    return TableAdamW(arena, lr=args.lr, betas=betas, eps=eps, weight_decay=args.weight_decay, layer_decay=layer_decay,
                      no_weight_decay=no_weight_decay or (), ema_decay=ema_decay)


def create_scheduler(args, optimizer):
    """Counterpart of ``timm.scheduler.create_scheduler(args, optimizer)`` -> (scheduler, num_epochs)."""
    if str(args.sched).lower() != "cosine":
        raise NotImplementedError(f"scheduler {args.sched!r}: only 'cosine' (every reference train_config) is implemented")
    sched = CosineLRScheduler(optimizer, t_initial=args.epochs, lr_min=args.min_lr, warmup_t=args.warmup_epochs,
                              warmup_lr_init=args.warmup_lr)
    return sched, args.epochs + (getattr(args, "cooldown_epochs", 0) or 0)
