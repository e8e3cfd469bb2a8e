"""Model factory, optimizer-argument adaptor and checkpoint I/O -- counterpart of the reference
``src/myrtle_vision/utils/models.py`` with the same signatures and the same checkpoint wire format
(``torch.save({"model", "optimizer", "lr_scheduler", "iteration"})``, utils/models.py:113-126).

DeiT distillation: a ``distiller_config`` gives (``DistillableViT``, ``DistillWrapper``) as in the reference (``models/distill.py``;
the reference's own forward is stale).  ``get_teacher`` keeps the reference's signature and its torchvision ResNet-50
(imported lazily; an ImportError names the alternative where torchvision is missing); the teacher that is built and tested here is a
``ViT`` of this package (``distiller_config["teacher_vit_config"]``).  Checkpoints of a distillation run carry one more key,
``"distiller"`` (token and head); ``"model"`` stays the student's state dict.
``rename_timm_state_dict`` cannot download timm weights offline; it converts a LOCAL timm-format state dict
(a ``.pth``/``.pt`` path or an in-memory dict) with the reference's renaming rules (utils/models.py:157-223).
"""
import argparse
import os
import re

import torch

from myrtle_vision.models.vit import ViT
from myrtle_vision.utils.quantize import QFormat
from myrtle_vision.utils.utils import parse_config


def _vit_kwargs(vit_config, num_classes, profile=False):
    """``ViT`` keyword arguments from a ``vit_config`` object (reference utils/models.py:29-42 and this package's extension keys)."""
    vit_kwargs = {
        "decoder": vit_config["decoder"],
        "image_size": vit_config["image_size"],
        "patch_size": vit_config["patch_size"],
        "num_classes": num_classes,
        "dim": vit_config["embed_dim"],
        "depth": vit_config["depth"],
        "heads": vit_config["heads"],
        "mlp_dim": vit_config["mlp_dim"],
        "dropout": vit_config["dropout"],
        "emb_dropout": vit_config["emb_dropout"],
        "profile": profile,
        "q_format": QFormat[vit_config["q_format"]],
        "precision": vit_config.get("precision"),
    }
    if vit_config.get("live_det_tokens"):
        vit_kwargs["live_det_tokens"] = True
    if vit_config.get("drop_path_rate") is not None:
        vit_kwargs["drop_path_rate"] = float(vit_config["drop_path_rate"])    # stochastic depth (an extension); absent -> 0.0
    if vit_config["decoder"] == "detection" and vit_config.get("num_det_tokens") is not None:
        vit_kwargs["num_det_tokens"] = vit_config["num_det_tokens"]    # the key the reference's yolos configs carry (default 100)
    return vit_kwargs


def get_teacher(num_classes, weights_path):
    """reference utils/models.py:14-22: the frozen ResNet-50 teacher of the reference's deit configs, from torchvision.  torchvision
    is imported here and not at module level: where it is missing this raises an ImportError naming the alternative, a ``ViT`` of
    this package (``distiller_config["teacher_vit_config"]``, ``get_vit_teacher``)."""
    try:
        from torchvision.models import resnet50
    except ImportError as e:
        raise ImportError("get_teacher builds the reference's ResNet-50 teacher and needs torchvision, which is not installed; "
                          "use a ViT teacher of this package instead: distiller_config['teacher_vit_config'] (a vit_config object) "
                          "with teacher_weights_path pointing at its checkpoint or state dict") from e
    teacher = resnet50(num_classes=num_classes)
    teacher.load_state_dict(torch.load(weights_path, map_location="cpu"))
    for param in teacher.parameters():
        param.requires_grad = False
    teacher.eval()
    return teacher


def get_vit_teacher(teacher_vit_config, num_classes, weights_path):
    """A frozen ``ViT`` of this package as the teacher (an extension: ``distiller_config["teacher_vit_config"]``).  ``weights_path``
    is a package checkpoint (its ``"model"`` entry is taken) or a bare state dict."""
    if not isinstance(weights_path, str) or not os.path.isfile(weights_path):
        raise FileNotFoundError(f"distiller_config['teacher_weights_path']={weights_path!r} is not a file: the teacher needs trained "
                                "weights (a checkpoint of this package or a state dict)")
    teacher = ViT(**_vit_kwargs(teacher_vit_config, num_classes))
    state = torch.load(weights_path, map_location="cpu", weights_only=False)
    if isinstance(state, dict) and isinstance(state.get("model"), dict):
        state = state["model"]
    teacher.load_state_dict(state)
    teacher.requires_grad_(False)
    teacher.eval()
    return teacher


_DISTILLER_KEYS = ("temperature", "alpha", "teacher_weights_path", "distillation_type", "teacher_vit_config")


def get_models(config, profile=False, with_teacher=True):
    """reference utils/models.py:25-60 -> (vit, distiller or None).  Optional extension keys ``vit_config["precision"]``,
    ``vit_config["drop_path_rate"]`` (stochastic depth, ``ViT(drop_path_rate=...)``; absent = 0.0) and, for
    ``decoder: "detection"``, ``vit_config["live_det_tokens"]`` (ViT's opt-in YOLOS sequence assembly; the criterion, matcher and
    post-processing live in ``myrtle_vision.models.detector`` / ``.matcher``).

    With a ``distiller_config`` (reference keys ``temperature``, ``alpha``, ``teacher_weights_path``) -> (``DistillableViT``,
    ``DistillWrapper``).  Extension keys: ``distillation_type`` (``"soft"``, the reference's loss, or ``"hard"``) and
    ``teacher_vit_config`` (a ``vit_config`` object: the teacher is a ``ViT`` of this package, ``get_vit_teacher``; without it the
    reference's torchvision ResNet-50, ``get_teacher``).  ``with_teacher=False`` (evaluation: the student alone is loaded and run)
    -> (``DistillableViT``, None) without touching the teacher or its file."""
    vit_config = config["vit_config"]
    data_config = parse_config(config["data_config_path"])
    if "distiller_config" in config:
        from myrtle_vision.models.distill import DistillableViT, DistillWrapper
        dc = config["distiller_config"]
        unknown = set(dc) - set(_DISTILLER_KEYS)
        if unknown:
            raise ValueError(f"distiller_config has unknown keys {sorted(unknown)} (known: {_DISTILLER_KEYS})")
        vit = DistillableViT(**_vit_kwargs(vit_config, data_config["number_of_classes"], profile))
        if not with_teacher:
            return vit, None
        if dc.get("teacher_vit_config") is not None:
            teacher = get_vit_teacher(dc["teacher_vit_config"], data_config["number_of_classes"], dc["teacher_weights_path"])
        else:
            teacher = get_teacher(num_classes=data_config["number_of_classes"], weights_path=dc["teacher_weights_path"])
        distiller = DistillWrapper(student=vit, teacher=teacher, temperature=dc["temperature"], alpha=dc["alpha"],
                                   distillation_type=dc.get("distillation_type", "soft"))
        return vit, distiller
    return ViT(**_vit_kwargs(vit_config, data_config["number_of_classes"], profile)), None


def prepare_model_and_load_ckpt(train_config, model, optimizer=None, lr_scheduler=None, distiller=None):
    """reference utils/models.py:63-81: resume when ``checkpoint_path`` is non-empty, else iteration 0."""
    if train_config["checkpoint_path"] != "":
        return load_checkpoint(model=model, optimizer=optimizer, lr_scheduler=lr_scheduler,
                               filepath=train_config["checkpoint_path"], distiller=distiller)
    return 0


def get_optimizer_args(train_config):
    """reference utils/models.py:84-110 (returns a namespace INSTANCE; the reference mutates the class)."""
    a = argparse.Namespace()
    a.opt = train_config["optimizer"]
    a.opt_eps = train_config["opt_eps"]
    a.opt_betas = train_config["opt_betas"]
    a.clip_grad = train_config["clip_grad"]
    a.momentum = train_config["momentum"]
    a.weight_decay = train_config["weight_decay"]
    a.sched = train_config["scheduler"]
    a.lr = train_config["lr"]
    a.lr_noise = train_config.get("lr_noise")
    a.lr_noise_pct = train_config.get("lr_noise_pct")
    a.lr_noise_std = train_config.get("lr_noise_std")
    a.warmup_lr = train_config["warmup_lr"]
    a.min_lr = train_config["min_lr"]
    a.epochs = train_config["epochs"]
    a.decay_epochs = train_config["decay_epochs"]
    a.warmup_epochs = train_config["warmup_epochs"]
    a.cooldown_epochs = train_config["cooldown_epochs"]
    a.patience_epochs = train_config["patience_epochs"]
    a.decay_rate = train_config["decay_rate"]
    # optional keys of the fine-tuning recipe (an extension, utils/optim.py TableAdamW): absent -> None -> the reference optimizer
    a.layer_decay = train_config.get("layer_decay")
    a.no_weight_decay = train_config.get("no_weight_decay")
    a.model_ema_decay = train_config.get("model_ema_decay")
    # "optimizer": "lamb" only (utils/optim.py TableLamb): the global gradient-norm clip timm's Lamb always makes; absent -> 1.0, its
    # default; null switches it off
    a.lamb_max_grad_norm = train_config.get("lamb_max_grad_norm", 1.0)
    return a


def save_checkpoint(model, optimizer, lr_scheduler, iteration, filepath, model_ema=None, distiller=None):
    """``model_ema`` (an extension): the weight EMA as a full model state dict (``TableAdamW.ema_state_dict``), written under
    ``"model_ema"``; None keeps the reference's four keys.  ``distiller`` (an extension, a ``DistillWrapper``): its
    ``distillation_token`` and ``distill_mlp.*`` go under ``"distiller"`` -- the reference saves the student alone
    (classification/train.py:217-224), so a run resumed there restarts the distillation head; ``"model"`` stays the student's state
    dict either way, loadable into a plain ``ViT``."""
    ckpt = {
        "model": {k: v.detach().cpu().clone() for k, v in model.state_dict().items()},
        "optimizer": optimizer.state_dict(),
        "lr_scheduler": lr_scheduler.state_dict(),
        "iteration": iteration,
    }
    if model_ema is not None:
        ckpt["model_ema"] = {k: v.detach().cpu().clone() for k, v in model_ema.items()}
    if distiller is not None:
        ckpt["distiller"] = distiller.head_state_dict()
    torch.save(ckpt, filepath)


def load_checkpoint(model, optimizer, lr_scheduler, filepath, use_ema=False, distiller=None):
    """``use_ema`` (evaluation): the model takes the checkpoint's ``"model_ema"`` instead of ``"model"``; a checkpoint without
    that key is an error.  An optimizer that keeps an EMA takes ``"model_ema"`` back when the checkpoint has one.  ``distiller``
    (a ``DistillWrapper``): takes the checkpoint's ``"distiller"`` entry back; a checkpoint without one (the reference's format)
    leaves the freshly initialised token and head, with a printed warning."""
    checkpoint = torch.load(filepath, map_location="cpu", weights_only=False)
    if distiller is not None:
        if "distiller" in checkpoint:
            distiller.load_head_state_dict(checkpoint["distiller"])
        else:
            print(f"WARNING: checkpoint {filepath!r} has no 'distiller' entry: the distillation token and head start fresh")
    if use_ema:
        if "model_ema" not in checkpoint:
            raise KeyError(f"use_ema: checkpoint {filepath!r} has no 'model_ema' entry (it was trained without model_ema_decay)")
        model.load_state_dict(checkpoint["model_ema"])
    else:
        model.load_state_dict(checkpoint["model"])
    if optimizer is not None:
        optimizer.load_state_dict(checkpoint["optimizer"])
        if getattr(optimizer, "ema", None) is not None and "model_ema" in checkpoint:
            optimizer.load_ema_state_dict(checkpoint["model_ema"])
    if lr_scheduler is not None:
        lr_scheduler.load_state_dict(checkpoint["lr_scheduler"])
    return checkpoint["iteration"]


def apply_rules(name, rules):
    """Apply the first matching rule (regex substitution) to name (reference utils/models.py:144-151)."""
    for pattern, replacement in rules:
        if re.match(pattern, name) is not None:
            return re.sub(pattern, replacement, name)
    return name


_BLOCK = r"blocks\.([0-9]+)\."
_TIMM_RULES = [
    (r"pos_embed", r"pos_embedding"),
    (r"patch_embed\.proj\.(weight|bias)", r"patch_to_embedding.\1"),
    (_BLOCK + r"norm1\.(weight|bias)", r"transformer.layers.\1.0.fn.norm.\2"),
    (_BLOCK + r"attn\.qkv\.(weight|bias)", r"transformer.layers.\1.0.fn.fn.to_qkv.\2"),
    (_BLOCK + r"attn\.proj\.(weight|bias)", r"transformer.layers.\1.0.fn.fn.to_out.0.\2"),
    (_BLOCK + r"norm2\.(weight|bias)", r"transformer.layers.\1.1.fn.norm.\2"),
    (_BLOCK + r"mlp\.fc1\.(weight|bias)", r"transformer.layers.\1.1.fn.fn.net.0.\2"),
    (_BLOCK + r"mlp\.fc2\.(weight|bias)", r"transformer.layers.\1.1.fn.fn.net.3.\2"),
]
_TIMM_HEAD = [r"norm\.weight", r"norm\.bias", r"head\.weight", r"head\.bias"]


def rename_timm_state_dict(timm_model_name, vit_config, num_classes):
    """timm ViT state dict -> this package's names (reference utils/models.py:154-223).

    ``timm_model_name`` is a local file path or an already loaded dict (the reference passes a model NAME and
    downloads it; there is no network here).  The classifier head (norm/head) is dropped and the conv patch
    embedding (O, I, H, W) is permuted to the Linear layout (O, (H, W, I))."""
    if isinstance(timm_model_name, dict):
        src = timm_model_name
    elif isinstance(timm_model_name, str) and os.path.exists(timm_model_name):
        src = torch.load(timm_model_name, map_location="cpu", weights_only=False)
        src = src.get("model", src.get("state_dict", src)) if isinstance(src, dict) else src
    else:
        raise FileNotFoundError(
            f"pretrained_backbone={timm_model_name!r}: timm checkpoints cannot be downloaded here; pass a path to a "
            "local timm-format state dict (or leave pretrained_backbone unset to train from random init)")
    out = {}
    for key, value in src.items():
        if any(re.match(p, key) for p in _TIMM_HEAD):
            continue
        new_key = apply_rules(key, _TIMM_RULES)
        if new_key == "patch_to_embedding.weight" and value.dim() == 4:
            patch_dim = vit_config["patch_size"] ** 2 * value.shape[1]
            value = value.permute(0, 2, 3, 1).reshape(vit_config["embed_dim"], patch_dim)
        out[new_key] = value
    return out
