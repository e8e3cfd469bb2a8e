"""Training / evaluation loops shared by the ``classification/``, ``segmentation/`` and ``detection/`` scripts.

Loop semantics follow the reference scripts (classification/train.py:55-313, segmentation/train.py, */test.py):
seeding, batch-size solver, one process per GPU, rank-0 checkpoints every ``iters_per_checkpoint`` iterations named
``vit_{iteration:06}``, rank-0 validation every ``iters_per_val``, gradient accumulation without dividing the loss,
``lr_scheduler.step(epoch)`` at epoch end.  Differences, all deliberate:

* compute runs on the HIP kernels (model, loss, optimizer); no CPU fallback;
* gradients are exchanged by ``utils.ddp.GradAllReducer`` over RCCL, and only on the LAST micro-batch of an
  accumulation window (the reference's DDP all-reduces every micro-batch; the result is identical) -- except when
  ``clip_grad`` is set with ``n_batch_accum > 1``: then every micro-batch is exchanged, because the reference clips the
  running accumulated (and already averaged) gradient after every backward, and that needs the averaged gradient each time;
* the two detection-only parameters are left out of the optimizer/all-reduce (the reference's DDP dies on them);
* ``GradScaler`` is dropped (a numerical no-op without autocast);
* ``clip_grad`` is the reference's ``clip_grad_norm_`` after EVERY micro-batch backward on the running accumulated gradient
  (classification/train.py:265-270): the intermediate clips rescale the gradient arena in place
  (``AdamW.clip_accumulated``), the last one rides into the AdamW kernel as a device scalar;
* with a ``distiller_config`` (DeiT distillation, classification/train.py:162-163,238-253) the student runs ONCE per step -- the
  training accuracy comes from the loss kernel's arg-max, where the reference runs the student a second time -- validation keeps the
  plain criterion on the student's class logits (the reference validates the distiller's loss, train.py:41-42), and the checkpoint
  gains a ``"distiller"`` entry (token and head; the reference drops them);
* ``pretrained_backbone`` must be a local timm-format state dict (no network); a bare timm model NAME that is not a
  file means "random init" with a warning.

Both loops share one skeleton: ``_begin`` (device, seed, batch sizes, process group, output directory), ``_model_and_optimizer``,
``_resume`` (checkpoint, reducer, broadcast, EMA start, first epoch) and one ``AccumWindow`` (zero_grad / exchange / clip / step).

``task="detection"`` follows detection/train.py:40-332 instead (``_train_detection``): padded batches of differently sized
images, ``SetCriterion`` weighted by ``train_config``'s ``weight_dict`` keys, validation on EVERY rank once per epoch
(``PostProcess`` -> ``CocoEvaluator`` -> validation loss) and a checkpoint ``vit_epoch{N}`` whenever AP@[.5:.95] does not drop.
"""
import os
import random
import time

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader, Sampler

from myrtle_vision.hip.functional import CrossEntropyLoss
from myrtle_vision.hip import ops
from myrtle_vision.utils.ddp import GradAllReducer, broadcast_parameters, exchange_dtype_from_env
from myrtle_vision.utils.miou import MIoU
from myrtle_vision.utils.models import (get_models, get_optimizer_args, prepare_model_and_load_ckpt,
                                        rename_timm_state_dict, save_checkpoint)
from myrtle_vision.utils.optim import create_optimizer, create_scheduler
from myrtle_vision.utils.utils import (cleanup_distributed, get_batch_sizes, init_distributed, parse_config,
                                       seed_everything)


class ShardSampler(Sampler):
    """Index for index what ``torch.utils.data.DistributedSampler(dataset)`` yields (classification/train.py:116,200:
    default arguments, so shuffle, seed 0, no drop_last): ``randperm(n)`` from a generator seeded ``seed + epoch``, padded
    to a multiple of the world size by repeating the head of the list, rank r takes ``indices[r::world]``
    (``tests/test_host_cpu.py::test_shard_sampler_is_torch_distributed_sampler``)."""

    def __init__(self, n, rank, world, seed=0, shuffle=True):
        self.n, self.rank, self.world, self.seed, self.epoch, self.shuffle = n, rank, world, seed, 0, shuffle
        self.num_samples = (n + world - 1) // world

    def set_epoch(self, epoch):
        self.epoch = epoch

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:                                                  # DistributedSampler(dataset, shuffle=False): detection/train.py:159
            idx = list(range(self.n))
        pad = self.num_samples * self.world - len(idx)
        if pad > 0:
            idx += (idx * -(-pad // len(idx)))[:pad]
        return iter(idx[self.rank::self.world])

    def __len__(self):
        return self.num_samples


def _datasets(task, data_config):
    if task == "detection":
        from myrtle_vision.datasets.coco import CocoDetection
        from myrtle_vision.datasets.detection_transforms import collate_fn, from_config

        def mk_det(split, ops_, plan=None):
            """``split``: "train" | "valid" | "test" (the ``<split>_images`` / ``<split>_annotations`` keys, detection/train.py:133-144)."""
            root = data_config["dataset_path"]
            return CocoDetection(img_folder=os.path.join(root, data_config[f"{split}_images"]),
                                 ann_file=os.path.join(root, "annotations", data_config[f"{split}_annotations"]),
                                 transforms=from_config(data_config[ops_]) if plan is None else None, device_plan=plan)
        return mk_det, collate_fn
    if task == "classification":
        from myrtle_vision.datasets.resisc45 import Resisc45 as DS
        collate = None
    else:
        from myrtle_vision.datasets.dlrsd import Dlrsd as DS, collate_both as collate
    mk = lambda mode, files, ops_, plan=None: DS(mode=mode, dataset_path=data_config["dataset_path"],
                                                 imagepaths=data_config[files], label_map_path=data_config["label_map"],
                                                 transform_config=data_config[ops_], device_plan=plan)
    return mk, collate


def _device_plan(data_config, ops_, enabled=True, task=None):
    """DevicePlan (DetectionDevicePlan for ``task="detection"``) for a ``transform_ops_*`` section, or None (host transforms)
    when disabled or the chain is not one the GPU path covers.  MYRTLE_VISION_DEVICE_TRANSFORMS=0 forces the host path."""
    if not enabled or os.environ.get("MYRTLE_VISION_DEVICE_TRANSFORMS", "1") == "0":
        return None
    from myrtle_vision.datasets.device_transforms import DetectionDevicePlan, DevicePlan
    try:
        return DetectionDevicePlan(data_config[ops_]) if task == "detection" else DevicePlan(data_config[ops_])
    except ValueError:
        return None


def _workers():
    """The reference uses one worker that also resizes/normalises; with those on the GPU the workers only decode, and
    there may be as many as this process's CPU share allows (capped: a 1-GPU job owns 16 cores)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 2
    return max(1, min(8, n - 2))


def _tensors_in(out):
    """Every tensor of a staged batch: (images, labels) for classification / segmentation, (NestedTensor, [target dict, ...])
    for detection."""
    if torch.is_tensor(out):
        yield out
    elif isinstance(out, dict):
        for v in out.values():
            yield from _tensors_in(v)
    elif isinstance(out, (list, tuple)):
        for v in out:
            yield from _tensors_in(v)
    elif hasattr(out, "decompose"):
        yield from _tensors_in(out.decompose())


class BatchFeed:
    """DataLoader -> (images fp32 [B,3,H,W], labels) ON THE DEVICE, for either path: host transforms (tensors are copied
    over) or a DevicePlan (uint8 frames + tables are copied over and mv_image_prepare / mv_mask_prepare finish the
    job).  Same batches either way (tests/test_image_prep.py).  ``task="detection"``: (NestedTensor [B,3,Hmax,Wmax] + padding
    mask, list of target dicts) instead, from the host collate or from a DetectionDevicePlan (mv_image_prepare_ragged /
    mv_image_resize_u8_ragged), same batches either way as well (tests/test_detection_data_gpu.py)."""

    def __init__(self, dataset, plan, task, device, collate, **loader_kw):
        self.plan, self.task, self.device = plan, task, device
        if plan is not None:
            loader_kw.setdefault("num_workers", _workers())
            collate = plan.collate
        else:
            loader_kw.setdefault("num_workers", 1)                          # classification/train.py:117
        # workers outlive the epoch: respawning them (fork + imports) costs seconds per epoch boundary, as long as ~90
        # iterations of ViT-B at batch 256
        loader_kw.setdefault("persistent_workers", loader_kw["num_workers"] > 0)
        self.loader = DataLoader(dataset, collate_fn=collate, pin_memory=True, **loader_kw)

    def __len__(self):
        return len(self.loader)

    def _to_device(self, batch):
        if self.task == "detection":                           # (NestedTensor, list of target dicts), both on the device
            first, targets = batch
            imgs = first.to(self.device) if self.plan is None else self.plan.apply(first, self.device)
            return imgs, [{k: v.to(self.device, non_blocking=True) for k, v in t.items()} for t in targets]
        if self.plan is None:
            imgs, labels = batch
            return imgs.to(self.device, non_blocking=True), labels.to(self.device, non_blocking=True)
        packed, labels = batch
        imgs, masks = self.plan.apply(packed, self.device, mask_add=-1 if self.task == "segmentation" else 0)
        return imgs, (masks if self.task == "segmentation" else labels.to(self.device, non_blocking=True))

    def __iter__(self):
        """One batch ahead on a side stream: the host-to-device copy (50 MB of uint8 frames for 256 images, ~2 ms of PCIe)
        and the image-preparation kernels of batch i+1 run under the model step of batch i instead of in front of it."""
        if torch.device(self.device).type != "cuda":
            for batch in self.loader:
                yield self._to_device(batch)
            return
        main, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)

        def stage(batch):
            with torch.cuda.stream(side):
                out = self._to_device(batch)
                ready = torch.cuda.Event()
                ready.record(side)
            for t in _tensors_in(out):
                t.record_stream(main)                # allocated on the side stream, consumed on the main one
            return out, ready

        it = iter(self.loader)
        try:
            cur = stage(next(it))
        except StopIteration:
            return
        while cur is not None:
            try:
                nxt = stage(next(it))                # queued now, so that it overlaps the step the caller runs on ``cur``
            except StopIteration:
                nxt = None
            out, ready = cur
            main.wait_event(ready)
            yield out
            cur = nxt


class _Scalars:
    """The reference's segmentation loop logs validation accuracy / loss / mIoU to TensorBoard
    (segmentation/train.py:17,33,69-71: ``SummaryWriter("runs/")``).  ``torch.utils.tensorboard`` needs the
    ``tensorboard`` package; where it is missing the same three scalars go to ``runs/scalars.jsonl`` instead (one JSON
    object per call), so the log exists either way and nothing fails at import time."""

    def __init__(self, logdir="runs/"):
        self.writer, self.path = None, None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.writer = SummaryWriter(logdir)
        except Exception:                                       # ImportError, or tensorboard present but unusable
            os.makedirs(logdir, exist_ok=True)
            self.path = os.path.join(logdir, "scalars.jsonl")

    def add_scalar(self, tag, value, step):
        if self.writer is not None:
            self.writer.add_scalar(tag, value, step)
        else:
            import json
            with open(self.path, "a") as f:
                f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")

    def close(self):
        if self.writer is not None:
            self.writer.close()


def _fused_seg_tail(task, criterion):
    """The segmentation loops may replace ``criterion(vit(x), y)`` + ``argmax`` by ``vit.segmentation_loss`` only when
    the criterion is the plain mean cross entropy the reference uses (segmentation/train.py:188)."""
    from myrtle_vision.hip.functional import CrossEntropyLoss
    return task == "segmentation" and type(criterion) is CrossEntropyLoss


_MIX_KEYS = ("label_smoothing", "mixup_alpha", "cutmix_alpha", "mixup_prob", "mixup_switch_prob")


def _train_criterion(task, train_config):
    """-> (training criterion, Mixup or None) from the optional ``train_config`` keys ``label_smoothing``, ``mixup_alpha``,
    ``cutmix_alpha``, ``mixup_prob`` (default 1) and ``mixup_switch_prob`` (default 0.5): an extension, the reference has no such
    recipe.  With smoothing and both alphas absent or zero this is the reference's ``CrossEntropyLoss()`` and no mixer, and
    ``utils.mixup`` is not even imported; otherwise ``SoftTargetCrossEntropy`` and, with an alpha > 0, a ``Mixup``.  Classification
    only: any of the keys on another task is an error."""
    present = [k for k in _MIX_KEYS if k in train_config]
    if present and task != "classification":
        raise ValueError(f"train_config key {present[0]!r} is a classification recipe (label smoothing / Mixup / CutMix); "
                         f"task={task!r} does not take it")
    smoothing = float(train_config.get("label_smoothing", 0.0))
    mixup_alpha, cutmix_alpha = float(train_config.get("mixup_alpha", 0.0)), float(train_config.get("cutmix_alpha", 0.0))
    if smoothing == 0.0 and mixup_alpha == 0.0 and cutmix_alpha == 0.0:
        return CrossEntropyLoss(), None
    from myrtle_vision.hip.functional import SoftTargetCrossEntropy
    mixer = None
    if mixup_alpha > 0 or cutmix_alpha > 0:
        from myrtle_vision.utils.mixup import Mixup
        mixer = Mixup(mixup_alpha, cutmix_alpha, prob=float(train_config.get("mixup_prob", 1.0)),
                      switch_prob=float(train_config.get("mixup_switch_prob", 0.5)))
    return SoftTargetCrossEntropy(smoothing, return_argmax=True), mixer


_ERASE_KEYS = ("reprob", "remode", "recount")


def _random_eraser(task, train_config):
    """-> ``RandomErasing`` or None from the optional ``train_config`` keys ``reprob`` (default 0), ``remode`` ("pixel" default,
    "rand" or "const") and ``recount`` (default 1, timm's ``min_count``), timm's names: an extension, the reference never erases.
    With ``reprob`` absent or 0 there is no eraser and ``utils.random_erasing`` is not even imported.  Classification only (masks
    and boxes of the other tasks would have to follow): any of the keys on another task is an error."""
    present = [k for k in _ERASE_KEYS if k in train_config]
    if present and task != "classification":
        raise ValueError(f"train_config key {present[0]!r} is a classification recipe (Random Erasing); task={task!r} does not "
                         "take it")
    if float(train_config.get("reprob", 0.0)) == 0.0:
        return None
    from myrtle_vision.utils.random_erasing import RandomErasing
    return RandomErasing(probability=float(train_config["reprob"]), mode=train_config.get("remode", "pixel"),
                         min_count=train_config.get("recount", 1))


_SEG_LOSS_KEYS = ("class_weights","label_smoothing", "dice_weight", "dice_smooth")


def _seg_loss_spec(task, train_config, num_classes=None):
    """-> ``SegLoss`` from the optional ``train_config["seg_loss"]`` object (keys ``class_weights``: a list of ``number_of_classes``
    floats or null, ``label_smoothing``, ``dice_weight``, ``dice_smooth``), or None without the key: an extension, the reference
    trains segmentation on the plain mean cross entropy.  Segmentation only -- the key on another task is an error -- and training
    only: validation and testing keep the plain criterion, so ``val_loss`` stays comparable between recipes."""
    if "seg_loss" not in train_config:
        return None
    if task != "segmentation":
        raise ValueError(f"train_config key 'seg_loss' is the segmentation recipe (class weights / label smoothing / Dice on the "
                         f"fused tail); task={task!r} does not take it")
    cfg = train_config["seg_loss"]
    if not isinstance(cfg, dict) or set(cfg) - set(_SEG_LOSS_KEYS):
        raise ValueError(f"train_config['seg_loss'] must be an object with keys among {_SEG_LOSS_KEYS}, got {cfg!r}")
    from myrtle_vision.hip.functional import SegLoss
    spec = SegLoss(class_weights=cfg.get("class_weights"), label_smoothing=cfg.get("label_smoothing", 0.0),
                   dice_weight=cfg.get("dice_weight", 0.0), dice_smooth=cfg.get("dice_smooth", 1.0))
    if num_classes is not None:
        spec.check_classes(num_classes)
    return spec


def _ema_state(optimizer, vit):
    """``save_checkpoint``'s ``model_ema``: the weight EMA (``train_config["model_ema_decay"]``, utils/optim.py TableAdamW) as a full
    model state dict, or None without an EMA."""
    return optimizer.ema_state_dict(vit) if optimizer.ema is not None else None


def _validate_twice(optimizer, validate):
    """-> (``validate("")`` on the weights, ``validate("_ema")`` on the weight EMA or None without one), in that order; the argument
    is the suffix of the metric names."""
    plain = validate("")
    if optimizer.ema is None:
        return plain, None
    with optimizer.ema_weights():
        return plain, validate("_ema")


def _begin(rank, num_gpus, train_config, dist_config):
    """What either loop does first after its recipe-key checks: device, seed, batch sizes (written back into the caller's
    ``train_config``), process group, output directory -> (device, world, batch_size, n_batch_accum, out_dir)."""
    if not torch.cuda.is_available():
        raise RuntimeError("training needs an MI355X: the myrtle_vision HIP path has no CPU fallback")
    device = torch.device("cuda", rank)
    torch.cuda.set_device(device)
    seed_everything(train_config["seed"])
    world = max(num_gpus, 1)
    batch_size, n_batch_accum = get_batch_sizes(train_config["local_batch_size"], num_gpus,
                                                train_config["global_batch_size"], verbose=(rank == 0))
    train_config["local_batch_size"] = batch_size
    train_config["global_batch_size"] = batch_size * n_batch_accum * world
    train_config["n_batch_accum"] = n_batch_accum
    if num_gpus > 1:
        init_distributed(rank, num_gpus, **dist_config)
    out_dir = train_config["output_directory"]
    if rank == 0:
        os.makedirs(out_dir, exist_ok=True)
        print("output directory:", out_dir)
    return device, world, batch_size, n_batch_accum, out_dir


_DISTILL_REFUSED_KEYS = ("layer_decay", "no_weight_decay", "model_ema_decay")


def _check_distiller_config(config, task="classification"):
    """A ``distiller_config`` beside a key it does not compose with yet: a ValueError that names the combination, before any device
    work.  ``layer_decay`` / ``no_weight_decay`` go by parameter NAME and ``model_ema_decay`` keeps a model state dict; none of them
    knows the ``student.`` prefix the parameters carry inside a ``DistillWrapper``.  The distillation token has no fake-quantiser
    stub, so ``q_format`` must be ``"FP32"``."""
    if "distiller_config" not in config:
        return
    if task != "classification":
        raise ValueError(f"distiller_config is the classification recipe (DeiT distillation); task={task!r} does not take it")
    for key in _DISTILL_REFUSED_KEYS:
        if config["train_config"].get(key) is not None:
            raise ValueError(f"train_config key {key!r} together with distiller_config is not supported: it goes by the plain model's "
                             "parameter names, which carry a 'student.' prefix inside the distiller")
    q_format = config["vit_config"].get("q_format", "FP32")
    if q_format != "FP32":
        raise ValueError(f"vit_config q_format={q_format!r} together with distiller_config is not supported: the distillation token "
                         "has no fake-quantiser stub (use q_format 'FP32')")


def _model_and_optimizer(rank, config, data_config, device):
    """After the loaders: the model (from a local ``pretrained_backbone`` if one is named) on the device, its optimizer and schedule
    -> (vit, optimizer, lr_scheduler, optimizer_args, distiller).  With a ``distiller_config`` the optimizer is built over the
    ``DistillWrapper`` (classification/train.py:162-163): student, distillation token and head; the frozen teacher has no trainable
    parameter and stays out of the arena, hence out of the gradient exchange and the parameter broadcast.  Else ``distiller`` is None."""
    train_config = config["train_config"]
    vit, distiller = get_models(config)
    backbone = train_config.get("pretrained_backbone")
    if backbone is not None:
        if isinstance(backbone, str) and os.path.exists(backbone):
            missing = vit.load_state_dict(rename_timm_state_dict(backbone, config["vit_config"], data_config["number_of_classes"]),
                                          strict=False)
            assert missing.unexpected_keys == []
        elif rank == 0:
            print(f"WARNING: pretrained_backbone={backbone!r} is not a local file (no network): training from random init")
    vit = vit.to(device)
    if distiller is not None:
        distiller = distiller.to(device)                       # the student is the same module: moved once
    optimizer_args = get_optimizer_args(train_config)
    # leaves out unused_parameter_names() (det tokens unless live) -- the model's, or the distiller's view of them
    optimizer = create_optimizer(optimizer_args, vit if distiller is None else distiller)
    lr_scheduler, _ = create_scheduler(optimizer_args, optimizer)
    return vit, optimizer, lr_scheduler, optimizer_args, distiller


class AccumWindow:
    """One gradient-accumulation window of ``n_batch_accum`` micro-batches, the same in every loop: ``zero_grad`` at its start; the
    exchange switched on for the LAST backward only -- or for every one when clipping between micro-batches (``clip_every``);
    ``finish`` + ``clip_accumulated`` after each backward but the last; ``finish`` + ``step`` after the last.

    ``clip_every`` is classification/train.py:265-270 (clip_grad_norm_ after EVERY backward, on the running accumulated gradient): the
    norm is taken over the flat (all-reduced) gradient arena; on the last micro-batch of a window the coefficient is applied inside
    the AdamW kernel, on the earlier ones the arena is rescaled in place (which needs the averaged gradient: those micro-batches are
    exchanged too, as the reference's DDP does on every backward).

    The window outlives the epoch: one opened by the last batches of an epoch is completed by the first batches of the next."""

    def __init__(self, optimizer, reducer, n_batch_accum, clip_every):
        self.optimizer, self.reducer, self.n_batch_accum, self.clip_every = optimizer, reducer, n_batch_accum, clip_every
        self.n_accum = 0

    @property
    def at_start(self):
        """No micro-batch of the current window has run: the only place for a checkpoint or a validation."""
        return self.n_accum == 0

    def backward(self, loss):
        """``loss.backward()`` inside the window's sequence -> whether this micro-batch ended in an optimizer step."""
        if self.n_accum == 0:
            self.optimizer.zero_grad()
        self.reducer.enabled = self.reducer.world > 1 and (self.clip_every or self.n_accum == self.n_batch_accum - 1)
        loss.backward()
        self.n_accum += 1
        if self.n_accum < self.n_batch_accum:
            if self.clip_every:
                self.reducer.finish()
                self.optimizer.clip_accumulated()
            return False
        self.n_accum = 0
        self.reducer.finish()
        self.optimizer.step()
        return True


def _resume(train_config, vit, optimizer, lr_scheduler, clip_grad, n_batch_accum, samples_per_iteration, n_train, num_gpus,
            distiller=None):
    """After the criterion: the checkpoint (if any), the reducer, rank 0's parameters to every rank, the EMA's start, the clipping
    set-up; then every rank waits for the others -> (iteration, the epoch it falls in, the accumulation window)."""
    iteration = prepare_model_and_load_ckpt(train_config=train_config, model=vit, optimizer=optimizer, lr_scheduler=lr_scheduler,
                                            distiller=distiller)
    optimizer.arena.bump_versions()
    reducer = GradAllReducer(optimizer.arena, exchange_dtype=exchange_dtype_from_env())   # MV_DDP_EXCHANGE=bf16: half-width, opt-in
    broadcast_parameters(optimizer.arena)
    if optimizer.ema is not None and not optimizer.ema_loaded:
        optimizer.reset_ema()                                  # the EMA starts from the weights, unless the checkpoint carried one
    optimizer.grad_scale = reducer.grad_scale
    optimizer.max_grad_norm = clip_grad
    window = AccumWindow(optimizer, reducer, n_batch_accum, clip_every=clip_grad is not None and n_batch_accum > 1)
    epoch_offset = max(0, int(samples_per_iteration * iteration / max(n_train, 1)))
    if num_gpus > 1:
        dist.barrier()
    return iteration, epoch_offset, window


@torch.no_grad()
def validation(val_loader, device, criterion, vit, task, num_classes):
    total_loss, total_acc, n = 0.0, 0.0, max(len(val_loader), 1)
    miou = MIoU(num_classes, device) if task == "segmentation" else None     # counted where the predictions are
    vit.eval()
    for imgs, labels in val_loader:                            # a BatchFeed: both already on the device
        if _fused_seg_tail(task, criterion):
            loss, acc, pred = vit.segmentation_loss(imgs, labels)        # no [B,C,H,W] logits
            total_loss += float(loss) / n
            total_acc += float(acc) / n
        else:
            outputs = vit(imgs)
            total_loss += float(criterion(outputs, labels)) / n
            pred = outputs.argmax(dim=1)
            total_acc += float((pred == labels).float().mean()) / n
        if miou is not None:
            miou.add_img(pred, labels)                         # three bincounts on the device; 17 numbers leave it
    vit.train()
    return total_loss, total_acc, (miou.get_miou() if miou is not None else None)


def train_worker(rank, num_gpus, config, task="classification"):
    if task == "detection":
        _seg_loss_spec(task, config["train_config"])           # the segmentation recipe key on this task: an error before any work
        _check_distiller_config(config, task)
        _random_eraser(task, config["train_config"])
        return _train_detection(rank, num_gpus, config)
    train_config = config["train_config"]
    data_config = parse_config(config["data_config_path"])
    train_criterion, mixer = _train_criterion(task, train_config)      # first: a recipe key on the wrong task fails before any work
    eraser = _random_eraser(task, train_config)
    _check_distiller_config(config, task)
    seg_spec = _seg_loss_spec(task, train_config, data_config["number_of_classes"])
    device, world, batch_size, n_batch_accum, out_dir = _begin(rank, num_gpus, train_config, config["dist_config"])

    mk, collate = _datasets(task, data_config)
    use_dev = train_config.get("device_transforms", True)
    plan_t, plan_v = _device_plan(data_config, "transform_ops_train", use_dev), _device_plan(data_config, "transform_ops_val", use_dev)
    trainset = mk("train", "train_files", "transform_ops_train", plan_t)
    valset = mk("eval", "valid_files", "transform_ops_val", plan_v)
    sampler = ShardSampler(len(trainset), rank, world) if num_gpus > 1 else None     # seed 0: the reference's default
    train_loader = BatchFeed(trainset, plan_t, task, device, collate, shuffle=(sampler is None), sampler=sampler,
                             batch_size=batch_size, drop_last=train_config["drop_last_batch"])
    val_loader = BatchFeed(valset, plan_v, task, device, collate, batch_size=batch_size,
                           drop_last=train_config["drop_last_batch"])

    vit, optimizer, lr_scheduler, optimizer_args, distiller = _model_and_optimizer(rank, config, data_config, device)
    # validation keeps the plain criterion; without a recipe key it IS the training criterion, the reference's CrossEntropyLoss()
    # (with a distiller too: the student's class logits against the labels, not the reference's distiller loss of
    # classification/train.py:41-42, so that val_loss stays comparable between recipes -- and the teacher never runs in validation)
    criterion = train_criterion if type(train_criterion) is CrossEntropyLoss else CrossEntropyLoss()
    iteration, epoch_offset, window = _resume(train_config, vit, optimizer, lr_scheduler, optimizer_args.clip_grad, n_batch_accum,
                                              batch_size * world, len(trainset), num_gpus, distiller=distiller)
    smoothing = getattr(train_criterion, "smoothing", 0.0)     # SoftTargetCrossEntropy's; the plain criterion has none
    scalars = _Scalars(train_config.get("tensorboard_dir", "runs/")) if (task == "segmentation" and rank == 0) else None
    num_classes = data_config["number_of_classes"]

    def validate(suffix):
        val = validation(val_loader, device, criterion, vit, task, num_classes)
        if scalars is not None:                                  # segmentation/train.py:69-71
            for tag, value in (("accuracy", val[1]), ("loss", val[0]), ("miou", val[2])):
                scalars.add_scalar(tag + suffix, value, iteration)
        return val

    vit.train()
    if distiller is not None:
        distiller.train()                                      # token and head; the teacher stays in eval mode
    last_val, last_val_ema = (0.0, 0.0, None), None
    for epoch in range(epoch_offset, train_config["epochs"]):
        epoch_loss = epoch_acc = 0.0
        train_miou = MIoU(num_classes, device) if seg_spec is not None else None
        if sampler is not None:
            sampler.set_epoch(epoch)
        for imgs, labels in train_loader:
            if iteration % train_config["iters_per_checkpoint"] == 0 and window.at_start and rank == 0:
                save_checkpoint(model=vit, optimizer=optimizer, lr_scheduler=lr_scheduler, iteration=iteration,
                                filepath=f"{out_dir}/vit_{iteration:06}", model_ema=_ema_state(optimizer, vit), distiller=distiller)
            if iteration % train_config["iters_per_val"] == 0 and window.at_start and rank == 0:
                last_val, last_val_ema = _validate_twice(optimizer, validate)    # the EMA's figures are logged beside the plain ones
            if eraser is not None:                               # classification only; DeiT's order: erase per image, then mix
                imgs = eraser(imgs)                              # in place, two launches; the teacher sees the erased batch too
            if distiller is not None:                           # DeiT distillation; the teacher sees the mixed batch, as in DeiT
                lam = 1.0
                if mixer is not None:
                    imgs, lam = mixer(imgs, labels)
                # ONE student pass: the arg-max for the accuracy comes from the loss kernel (the reference runs the student twice,
                # classification/train.py:247-253)
                loss, pred = distiller(imgs, labels, lam=lam, smoothing=smoothing, pair_flip=mixer is not None, return_argmax=True)
                acc_t = (pred == labels).float().mean()
            elif seg_spec is not None:                           # class weights / smoothing / Dice: the fused tail or an error
                loss, acc_t, _, areas = vit.segmentation_loss(imgs, labels, loss=seg_spec, return_areas=True)
                train_miou.add_areas(areas)                      # counted by the loss kernel: no second pass, no synchronisation
            elif _fused_seg_tail(task, criterion):
                loss, acc_t, _ = vit.segmentation_loss(imgs, labels)
            elif train_criterion is criterion:
                outputs = vit(imgs)
                loss = criterion(outputs, labels)
                acc_t = None
            else:                                                # label smoothing / Mixup / CutMix: each micro-batch within itself
                lam = 1.0
                if mixer is not None:
                    imgs, lam = mixer(imgs, labels)              # in place; the labels stay the original ones
                loss, pred = train_criterion(vit(imgs), labels, lam)
                acc_t = (pred == labels).float().mean()          # the kernel's arg-max against the ORIGINAL labels
            if window.backward(loss):
                iteration += 1
                if rank == 0:
                    acc = float(acc_t) if acc_t is not None else float((outputs.argmax(dim=1) == labels).float().mean())
                    epoch_loss += float(loss.detach()) / len(train_loader)
                    epoch_acc += acc / len(train_loader)
                    print(f"Iteration {iteration}:\tloss={float(loss.detach()):.4f}\tacc={acc:.4f}")
        lr_scheduler.step(epoch)
        if rank == 0:
            extra = f" - val_miou: {last_val[2]:.4f}" if last_val[2] is not None else ""
            if train_miou is not None:                           # this rank's batches of the epoch
                extra = f" - train_miou: {train_miou.get_miou():.4f}" + extra
            if last_val_ema is not None:
                extra += f" - val_loss_ema : {last_val_ema[0]:.4f} - val_acc_ema: {last_val_ema[1]:.4f}"
                if last_val_ema[2] is not None:
                    extra += f" - val_miou_ema: {last_val_ema[2]:.4f}"
            print(f"Epoch : {epoch + 1} - loss : {epoch_loss:.4f} - acc: {epoch_acc:.4f} - "
                  f"val_loss : {last_val[0]:.4f} - val_acc: {last_val[1]:.4f}{extra}\n")
    if scalars is not None:
        scalars.close()
    if num_gpus > 1:
        cleanup_distributed()
    return iteration


def launch_training(config, task):
    """``__main__`` of the reference train scripts: timestamped output dir, one process per visible GPU."""
    from datetime import datetime
    import torch.multiprocessing as mp
    config["train_config"]["output_directory"] += datetime.now().strftime("_%m_%d_%Y_%H_%M_%S")
    num_gpus = torch.cuda.device_count()
    if config["train_config"]["distributed"]:
        if num_gpus <= 1:
            print(f"WARNING: tried to enable distributed training but only found {num_gpus} GPU(s)")
    elif num_gpus > 1:
        print("INFO: you have multiple GPUs available but did not enable distributed training")
        num_gpus = 1
    try:
        if num_gpus > 1:
            mp.spawn(train_worker, args=(num_gpus, config, task), nprocs=num_gpus, join=True)
        else:
            train_worker(0, num_gpus, config, task)
    except KeyboardInterrupt:
        print("Ctrl-c pressed; cleaning up and ending training early...")


@torch.no_grad()
def evaluate(config, task, quantize=False, calib_steps=0, quantized_ckpt=False):
    """classification/test.py, segmentation/test.py and classification/test_quantize.py in one function."""
    from myrtle_vision.utils.models import load_checkpoint
    from myrtle_vision.utils.quantize import QFormat
    train_config, vit_config = config["train_config"], config["vit_config"]
    data_config = parse_config(config["data_config_path"])
    vit_config["dropout"], vit_config["emb_dropout"] = 0.0, 0.0            # classification/test.py:47-48
    if train_config["checkpoint_path"] == "":
        raise ValueError("a checkpoint is required for evaluation (train_config.checkpoint_path)")
    q_format = vit_config["q_format"]
    if quantize and not quantized_ckpt:
        vit_config["q_format"] = "FP32"                                    # test_quantize.py:90-94: build FP32, load, then prepare
    vit, _ = get_models(config, with_teacher=False)            # a distillation run is evaluated on its student: no teacher file needed
    vit = vit.to("cuda")
    # "use_ema": true (top level or in train_config): evaluate the weight EMA the checkpoint carries under "model_ema"
    use_ema = bool(config.get("use_ema", train_config.get("use_ema", False)))
    load_checkpoint(model=vit, optimizer=None, lr_scheduler=None, filepath=train_config["checkpoint_path"], use_ema=use_ema)
    mk, collate = _datasets(task, data_config)
    dev = torch.device("cuda")
    if task == "detection":
        if quantize:
            raise NotImplementedError("quantised evaluation is a classification script (classification/test_quantize.py)")
        return _evaluate_detection(vit, mk, collate, data_config, train_config, dev)
    plan = _device_plan(data_config, "transform_ops_val", train_config.get("device_transforms", True))
    if quantize:
        if not quantized_ckpt:
            vit.quantizer.prepare_qat(q_format)
        calib = BatchFeed(mk("eval", "valid_files", "transform_ops_val", plan), plan, task, dev, collate,
                          batch_size=train_config["local_batch_size"])
        vit.train()
        for step, (imgs, _) in enumerate(calib):                           # test_quantize.py:26-34
            if step >= calib_steps:
                break
            vit(imgs)
        vit.convert()
    testset = mk("eval" if task == "classification" else "test", "test_files", "transform_ops_val", plan)
    loader = BatchFeed(testset, plan, task, dev, collate, batch_size=train_config["local_batch_size"])
    vit.eval()
    # predictions, the hit count and the mIoU histograms stay on the device (the reference concatenates int64 predictions and
    # labels of the whole test set on the host: 206 MB per batch of 256 masks); the segmentation decoder goes through the
    # fused tail, which yields the arg-max without the [B, C, H, W] logits
    miou = MIoU(data_config["number_of_classes"], dev) if task == "segmentation" else None
    correct, total = torch.zeros((), dtype=torch.float64, device=dev), 0
    preds, gts = [], []                                    # classification only (one label per image): for the report
    with torch.no_grad():
        for imgs, labels in loader:
            if task == "segmentation" and hasattr(vit, "segmentation_loss"):
                pred = vit.segmentation_loss(imgs, labels)[2]
            else:
                pred = vit(imgs).argmax(dim=1)
            correct += (pred == labels).sum()
            total += labels.numel()
            if miou is not None:
                miou.add_img(pred, labels)
            else:
                preds.append(pred.reshape(-1).cpu())
                gts.append(labels.reshape(-1).cpu())
    acc = float(correct) / max(total, 1)
    if miou is None:
        preds, gts = torch.cat(preds), torch.cat(gts)
    result = {"accuracy": acc}
    if miou is not None:
        result["miou"] = miou.get_miou()
        print(f"pixel accuracy: {acc:.4f}  mIoU: {result['miou']:.4f}")
    else:
        try:
            from sklearn.metrics import classification_report
            print(classification_report(gts.numpy(), preds.numpy(), digits=4, zero_division=0))
        except ImportError:
            print(f"accuracy: {acc:.4f}")
    return result


# ---- detection (detection/train.py, detection/test.py) ----------------------------------------------------------------
_DET_WEIGHTS = ("loss_ce", "class_error", "loss_bbox", "loss_giou", "cardinality_error")


def _weighted(losses, weight_dict):
    return sum(losses[k] * weight_dict[k] for k in losses.keys() if k in weight_dict)


def _random_subset(dataset, k):
    """detection/train.py:126-146: the first k of a ``random.shuffle`` of the indices."""
    from torch.utils.data import Subset
    perm = list(range(len(dataset)))
    random.shuffle(perm)
    return Subset(dataset, perm[:k])


class _JsonLines:
    """The detection loop's record (the reference logs lr and AP to TensorBoard, detection/train.py:321-323): one JSON object per
    iteration (``iteration``, ``loss``) and per epoch (``epoch``, ``loss``, ``val_loss``, ``ap``, ``lr``), floats at full precision."""

    def __init__(self, path):
        self.path = path

    def write(self, **row):
        import json
        with open(self.path, "a") as f:
            f.write(json.dumps(row) + "\n")


def _loss_to_host(loss, criterion):
    """The loss scalar on the host.  With the device-mode matcher (``train_config["device_matcher"]``) the solver's per-image
    status comes along in the same copy (0, 1 and 2 are exact in fp32), so checking it adds no synchronisation and no copy of its
    own; scipy's message is raised for an unsolved image."""
    status = getattr(criterion, "match_status", None)
    if status is None:
        return float(loss.detach())
    from myrtle_vision.models.matcher import raise_for_status
    both = torch.cat((loss.detach().reshape(1).float(), status.float())).cpu()
    raise_for_status(both[1:].to(torch.int32).numpy())
    return float(both[0])


@torch.no_grad()
def detection_validation(coco, val_loader, criterion, weight_dict, vit, verbose=True):
    """detection/train.py:40-71 -> (validation loss, AP@[.5:.95], the evaluator).  Runs on every rank: the criterion
    all-reduces the box count and the evaluator gathers the per-image records."""
    from myrtle_vision.datasets.coco_eval import CocoEvaluator
    from myrtle_vision.models.detector import PostProcess
    evaluator, post = CocoEvaluator(coco, ["bbox"]), PostProcess()
    total, n = 0.0, max(len(val_loader), 1)
    vit.eval()
    criterion.eval()
    for imgs, targets in val_loader:
        outputs = vit(imgs.tensors)
        sizes = torch.stack([t["orig_size"] for t in targets])
        results = post(outputs, sizes)
        evaluator.update({int(t["image_id"].item()): r for t, r in zip(targets, results)})
        total += _loss_to_host(_weighted(criterion(outputs, targets), weight_dict), criterion) / n
    evaluator.synchronize_between_processes()
    evaluator.accumulate()
    evaluator.summarize(verbose)
    vit.train()
    criterion.train()
    return total, float(evaluator.coco_eval["bbox"].stats[0]), evaluator


def _train_detection(rank, num_gpus, config):
    from myrtle_vision.datasets.coco import coco_from_dataset
    from myrtle_vision.models.detector import SetCriterion
    from myrtle_vision.models.matcher import HungarianMatcher
    train_config = config["train_config"]
    data_config = parse_config(config["data_config_path"])
    device, world, batch_size, n_batch_accum, out_dir = _begin(rank, num_gpus, train_config, config["dist_config"])

    mk, collate = _datasets("detection", data_config)
    use_dev = train_config.get("device_transforms", True)
    plan_t = _device_plan(data_config, "transform_ops_train", use_dev, "detection")
    plan_v = _device_plan(data_config, "transform_ops_val", use_dev, "detection")
    trainset = mk("train", "transform_ops_train", plan_t)
    if data_config.get("train_subset") is not None:
        trainset = _random_subset(trainset, data_config["train_subset"])
    valset = mk("valid", "transform_ops_val", plan_v)
    if data_config.get("valid_subset") is not None:
        valset = _random_subset(valset, data_config["valid_subset"])
    sampler = ShardSampler(len(trainset), rank, world) if num_gpus > 1 else None
    val_sampler = ShardSampler(len(valset), rank, world, shuffle=False) if num_gpus > 1 else None
    train_loader = BatchFeed(trainset, plan_t, "detection", device, collate, shuffle=(sampler is None), sampler=sampler,
                             batch_size=batch_size, drop_last=train_config["drop_last_batch"])
    val_loader = BatchFeed(valset, plan_v, "detection", device, collate, sampler=val_sampler, batch_size=batch_size,
                           drop_last=train_config["drop_last_batch"])

    vit, optimizer, lr_scheduler, optimizer_args, _ = _model_and_optimizer(rank, config, data_config, device)
    weight_dict = {k: train_config[k] for k in _DET_WEIGHTS if k in train_config}     # an absent key is left out of the sum
    # "device_matcher": the assignment in HIP (mv_det_match) instead of scipy on the host; training and validation share it
    matcher = HungarianMatcher(assignment="device" if train_config.get("device_matcher", False) else "host")
    criterion = SetCriterion(data_config["number_of_classes"], matcher=matcher, weight_dict=weight_dict,
                             eos_coef=train_config["eos_coef"], losses=["labels", "boxes", "cardinality"]).to(device)
    iteration, epoch_offset, window = _resume(train_config, vit, optimizer, lr_scheduler, optimizer_args.clip_grad, n_batch_accum,
                                              batch_size * world, len(trainset), num_gpus)

    def validate(suffix):                                      # on every rank, the EMA's too: the evaluator gathers
        val_loss, ap, _ = detection_validation(coco_from_dataset(valset), val_loader, criterion, weight_dict, vit, verbose=(rank == 0))
        return {"val_loss" + suffix: val_loss, "ap" + suffix: ap}

    vit.train()
    criterion.train()
    top_ap = 0.0
    log = _JsonLines(os.path.join(out_dir, "train_log.jsonl")) if rank == 0 else None
    for epoch in range(epoch_offset, train_config["epochs"]):
        epoch_loss = 0.0
        if sampler is not None:
            sampler.set_epoch(epoch)
        for imgs, targets in train_loader:                     # every batch may have a new (H, W): no captured graph here
            loss = _weighted(criterion(vit(imgs.tensors), targets), weight_dict)
            stepped = window.backward(loss)
            value = _loss_to_host(loss, criterion)
            epoch_loss += value / max(len(train_loader), 1)
            if stepped:
                iteration += 1
                if rank == 0:
                    print(f"Iteration {iteration}:\tloss={value:.4f}")
                    log.write(iteration=iteration, loss=value)
        if rank == 0:
            print(f"Epoch {epoch} validation...")
        row, ema_row = _validate_twice(optimizer, validate)
        val_loss, ap = row["val_loss"], row["ap"]
        if ap >= top_ap and rank == 0:
            save_checkpoint(model=vit, optimizer=optimizer, lr_scheduler=lr_scheduler, iteration=iteration,
                            filepath=f"{out_dir}/vit_epoch{epoch}", model_ema=_ema_state(optimizer, vit))
        top_ap = max(top_ap, ap)
        lr_scheduler.step(epoch)
        if rank == 0:
            log.write(epoch=epoch, loss=epoch_loss, val_loss=val_loss, ap=ap, lr=optimizer.param_groups[0]["lr"], **(ema_row or {}))
            print(f"Epoch : {epoch + 1} - loss : {epoch_loss:.4f} - val_loss : {val_loss:.4f} - val_acc: {ap:.4f}\n")
    if num_gpus > 1:
        cleanup_distributed()
    return iteration


def _evaluate_detection(vit, mk, collate, data_config, train_config, dev):
    """detection/test.py:29-73: the test split through the validation chain -> COCO bbox statistics."""
    from myrtle_vision.datasets.coco_eval import CocoEvaluator
    from myrtle_vision.models.detector import PostProcess
    plan = _device_plan(data_config, "transform_ops_val", train_config.get("device_transforms", True), "detection")
    testset = mk("test", "transform_ops_val", plan)
    loader = BatchFeed(testset, plan, "detection", dev, collate, batch_size=train_config["local_batch_size"],
                       drop_last=train_config["drop_last_batch"])
    evaluator, post = CocoEvaluator(testset.coco, ["bbox"]), PostProcess()
    vit.eval()
    for imgs, targets in loader:
        results = post(vit(imgs.tensors), torch.stack([t["orig_size"] for t in targets]))
        evaluator.update({int(t["image_id"].item()): r for t, r in zip(targets, results)})
    evaluator.synchronize_between_processes()
    evaluator.accumulate()
    evaluator.summarize()
    stats = [float(v) for v in evaluator.coco_eval["bbox"].stats]
    return {"AP": stats[0], "stats": stats}
