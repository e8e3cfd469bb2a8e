"""Layer-wise learning-rate decay, ``no_weight_decay`` and the weight EMA without a GPU: the layer ids and scales, the work-item
builder (as a property test), the config handling, the C ABI of ``mv_adamw_table`` (header, ``SIGNATURES``, export, argument checks
answered on the host) and the checkpoint keys."""
import argparse
import ctypes
import json
import os
import random
import re

import pytest
import torch

from conftest import ROOT
from optim_table_ref import EDGE_SIZES, ITEM_MAX, arena_offsets, gap_mask

HEADER = os.path.join(ROOT, "include", "myrtle_vision_hip.h")
OK, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -4
ADDR = 1 << 20                                               # 16-byte aligned, never read: every call below ends at its checks

VITS = {
    "classification": dict(decoder="classification", num_classes=5),
    "segmentation": dict(decoder="segmentation", num_classes=5),
    "detection": dict(decoder="detection", num_classes=5, live_det_tokens=True, num_det_tokens=10),
}


def _vit(task, depth=2):
    from myrtle_vision.models.vit import ViT
    return ViT(image_size=224, patch_size=16, dim=64, depth=depth, heads=1, mlp_dim=128, **VITS[task])


# ---------------------------------------------------------------- layer ids and scales
@pytest.mark.parametrize("task", list(VITS))
def test_layer_ids_and_scales(task):
    from myrtle_vision.utils.optim import layer_ids, layer_scales, vit_depth
    depth, decay = 2, 0.75
    names = [n for n, _ in _vit(task, depth).named_parameters()]
    assert vit_depth(names) == depth
    ids = layer_ids(names)
    assert len(ids) == len(names) and all(isinstance(i, int) and 0 <= i <= depth + 1 for i in ids)     # every parameter gets an id
    assert ids == sorted(ids)                                                   # monotone in module order
    by = dict(zip(names, ids))
    for n in ("pos_embedding", "cls_token", "patch_to_embedding.weight", "patch_to_embedding.bias", "det_tokens", "pos_embedding_det"):
        assert by[n] == 0, n
    for n in names:
        if n.startswith("transformer.layers."):
            assert by[n] == int(n.split(".")[2]) + 1
        elif n.startswith("decoder."):
            assert by[n] == depth + 1
    assert set(ids) == set(range(depth + 2))
    scales = dict(zip(names, layer_scales(names, decay)))
    head = [n for n in names if n.startswith("decoder.")]
    assert head and all(scales[n] == 1.0 for n in head)                         # exactly 1
    assert scales["pos_embedding"] == scales["cls_token"] == scales["patch_to_embedding.weight"] == decay ** (depth + 1)
    assert scales["transformer.layers.0.0.fn.norm.weight"] == decay ** depth
    assert scales["transformer.layers.1.0.fn.norm.weight"] == decay ** (depth - 1)
    assert all(s == 1.0 for s in layer_scales(names, 1.0))


# ---------------------------------------------------------------- no_weight_decay
def _table_opt(vit, **kw):
    from myrtle_vision.utils.optim import ParamArena, TableAdamW
    return TableAdamW(ParamArena(vit.named_parameters(), skip=vit.unused_parameter_names()), lr=1e-3, weight_decay=0.05, **kw)


def test_no_weight_decay_accepts_model_names_and_rejects_others():
    vit = _vit("classification")
    opt = _table_opt(vit, no_weight_decay=["pos_embedding", "cls_token"])
    wd = dict(zip(opt.arena.names, opt.tensor_weight_decays()))
    assert wd["pos_embedding"] == 0.0 and wd["cls_token"] == 0.0
    assert wd["patch_to_embedding.weight"] == 0.05 and wd["patch_to_embedding.bias"] == 0.0 and wd["decoder.linear.weight"] == 0.05
    plain = _table_opt(_vit("classification"), layer_decay=1.0)
    assert plain.arena.names == opt.arena.names and plain.arena.offsets == opt.arena.offsets     # the layout does not change
    assert plain.arena.n_decay == opt.arena.n_decay
    assert dict(zip(plain.arena.names, plain.tensor_weight_decays()))["pos_embedding"] == 0.05
    assert sorted(opt.segments) == [(1.0, 0.0), (1.0, 0.05)]                    # distinct pairs become segments
    with pytest.raises(ValueError, match="pos_embed_typo"):
        _table_opt(_vit("classification"), no_weight_decay=["pos_embedding", "pos_embed_typo"])
    _table_opt(_vit("classification"), no_weight_decay=["det_tokens"])          # a parameter of the model that the arena leaves out


# ---------------------------------------------------------------- the item builder, as a property test
def _check_items(sizes, pairs):
    from myrtle_vision.utils.optim import build_items
    offsets, total = arena_offsets(sizes)
    off, length, seg, segments = build_items(offsets, sizes, pairs)
    assert len(off) == len(length) == len(seg)
    assert len(set(segments)) == len(segments) and set(segments) == {(float(a), float(b)) for a, b in pairs}
    owner = torch.full((total,), -1, dtype=torch.int64)
    for t, (o, n) in enumerate(zip(offsets, sizes)):
        owner[o:o + n] = t
    hits = torch.zeros(total, dtype=torch.int64)
    for o, n, s in zip(off, length, seg):
        assert 1 <= n <= ITEM_MAX                                               # never more than 4096 elements
        assert o % 8 == 0                                                       # 32-byte aligned start
        hits[o:o + n] += 1
        t = int(owner[o])
        assert t >= 0 and bool((owner[o:o + n] == t).all())                     # never crosses a tensor, never touches a gap
        assert (o - offsets[t]) % ITEM_MAX == 0                                 # tensor offset + a multiple of 4096
        assert segments[s] == (float(pairs[t][0]), float(pairs[t][1]))          # the right segment
    gaps = gap_mask(offsets, sizes, total)
    assert bool((hits[~gaps] == 1).all()) and bool((hits[gaps] == 0).all())     # every tensor element exactly once, no gap element
    assert off == sorted(off)


def test_item_builder_covers_every_element_once():
    rng = random.Random(1234)
    must = [1, 3, 5, 8, 4095, 4096, 4097, 2 * 4096 + 5]
    pairs_pool = [(s, w) for s in (1.0, 0.75, 0.5625, 0.421875, 0.31640625) for w in (0.0, 0.05)]
    for trial in range(25):
        sizes = must + [rng.choice(EDGE_SIZES + [2, 4, 6, 16, 100, 12289]) for _ in range(rng.randint(0, 30))]
        rng.shuffle(sizes)
        pairs = [rng.choice(pairs_pool[: rng.randint(1, len(pairs_pool))]) for _ in sizes]
        _check_items(sizes, pairs)
    _check_items([1], [(1.0, 0.0)])
    _check_items([4096, 4096], [(1.0, 0.0), (1.0, 0.0)])


# ---------------------------------------------------------------- config handling
def _args(**extra):
    from myrtle_vision.utils.models import get_optimizer_args
    cfg = json.load(open(os.path.join(ROOT, "classification", "train_configs", "vit_tiny.json")))["train_config"]
    cfg.update(extra)
    return get_optimizer_args(cfg)


def test_absent_keys_build_the_plain_optimizer():
    from myrtle_vision.utils.optim import AdamW, create_optimizer
    args = _args()
    assert args.layer_decay is None and args.no_weight_decay is None and args.model_ema_decay is None
    opt = create_optimizer(args, _vit("classification"))
    assert type(opt) is AdamW
    for attr in ("items", "seg_lr_scale", "seg_wd", "lr_scales"):
        assert not hasattr(opt, attr), attr                                     # no table attributes in use
    assert opt.ema is None and "ema" not in vars(opt)                           # no EMA buffer: only the class's "none" answer
    opt = create_optimizer(argparse.Namespace(opt="adamw", lr=1e-3, weight_decay=0.05), _vit("classification"))
    assert type(opt) is AdamW                                                   # a namespace from before the keys existed


@pytest.mark.parametrize("key,value", [("layer_decay", 0.75), ("layer_decay", 1.0), ("no_weight_decay", ["pos_embedding"]),
                                       ("no_weight_decay", []), ("model_ema_decay", 0.999)])
def test_each_key_alone_switches_the_table_path_on(key, value):
    from myrtle_vision.utils.optim import AdamW, CosineLRScheduler, TableAdamW, create_optimizer
    opt = create_optimizer(_args(**{key: value}), _vit("classification"))
    assert type(opt) is TableAdamW and isinstance(opt, AdamW)
    assert opt.items[0].dtype == torch.int64 and opt.items[1].dtype == torch.int32 and opt.items[2].dtype == torch.int32
    assert (opt.ema is not None) == (key == "model_ema_decay")
    assert [g["name"] for g in opt.param_groups] == ["decay", "no_decay"]       # the two reference groups, one base rate
    sched = CosineLRScheduler(opt, t_initial=10, lr_min=1e-6, warmup_t=2, warmup_lr_init=1e-7)
    sched.step(5)
    assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] != opt.defaults["lr"]
    if key == "model_ema_decay":
        assert torch.equal(opt.ema, opt.arena.flat_param)                       # starts from the weights


@pytest.mark.parametrize("key,value", [("layer_decay", 0.0), ("layer_decay", 1.5), ("layer_decay", -0.1), ("layer_decay", float("nan")),
                                       ("layer_decay", "0.75"), ("model_ema_decay", 0.0), ("model_ema_decay", 1.0),
                                       ("model_ema_decay", 1.2), ("model_ema_decay", float("nan")), ("no_weight_decay", "pos_embedding"),
                                       ("no_weight_decay", ["pos_embedding", 3]), ("no_weight_decay", ["not_a_parameter"])])
def test_out_of_range_values_raise_with_the_keys_name(key, value):
    from myrtle_vision.utils.optim import create_optimizer
    with pytest.raises(ValueError, match=key):
        create_optimizer(_args(**{key: value}), _vit("classification"))


def test_shipped_config_parses_and_names_exist_in_vit_base():
    from myrtle_vision.models.vit import ViT
    from myrtle_vision.utils.models import get_optimizer_args
    from myrtle_vision.utils.optim import _check_unit, layer_scales
    d = os.path.join(ROOT, "classification", "train_configs")
    cfg, base = json.load(open(os.path.join(d, "vit_base_finetune.json"))), json.load(open(os.path.join(d, "vit_base_mixup.json")))
    extra = {k: v for k, v in cfg["train_config"].items() if k not in base["train_config"]}
    assert extra == {"layer_decay": 0.75, "no_weight_decay": ["pos_embedding", "cls_token"], "model_ema_decay": 0.9998}
    assert {k: v for k, v in cfg["train_config"].items() if k not in extra} == base["train_config"]
    assert cfg["vit_config"] == base["vit_config"]
    args = get_optimizer_args(cfg["train_config"])
    _check_unit("layer_decay", args.layer_decay)
    _check_unit("model_ema_decay", args.model_ema_decay, hi_closed=False)
    v = cfg["vit_config"]
    with torch.device("meta"):                                                  # names and shapes only: no 86 M element allocation
        vit = ViT(decoder=v["decoder"], image_size=v["image_size"], patch_size=v["patch_size"], num_classes=45, dim=v["embed_dim"],
                  depth=v["depth"], heads=v["heads"], mlp_dim=v["mlp_dim"])
    names = [n for n, _ in vit.named_parameters()]
    assert set(args.no_weight_decay) <= set(names)
    scales = layer_scales(names, args.layer_decay)
    assert min(scales) == 0.75 ** 13 and max(scales) == 1.0


# ---------------------------------------------------------------- C ABI
def test_header_signatures_and_library_carry_the_entry_point():
    from myrtle_vision.hip import build, lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+mv_adamw_table\s*\(", src)
    assert lib.SIGNATURES["mv_adamw_table"] == ("ppppp" "ppp" "l" "pp" "i" "p" "fffffff" "p" "f" "p", ctypes.c_int)
    assert hasattr(lib.lib(), "mv_adamw_table")
    assert "optim_table.hip" in build.SOURCES
    from myrtle_vision.hip import ops
    assert callable(ops.adamw_table_step)


def _call(p=ADDR, g=ADDR, m=ADDR, v=ADDR, ema=None, off=ADDR, length=ADDR, seg=ADDR, n_items=4, scale=ADDR, wd=ADDR, n_seg=2,
          hyper=None, beta1=0.9, beta2=0.999, ema_decay=0.0):
    from myrtle_vision.hip import lib
    return lib.lib().mv_adamw_table(p, g, m, v, ema, off, length, seg, n_items, scale, wd, n_seg, hyper, 1e-3, beta1, beta2, 1e-8,
                                    0.1, 0.001, 1.0, None, ema_decay, None)


@pytest.mark.parametrize("kw,code", [
    (dict(p=None), ALIGN), (dict(g=None), ALIGN), (dict(m=None), ALIGN), (dict(v=None), ALIGN),
    (dict(p=ADDR + 4), ALIGN), (dict(g=ADDR + 8), ALIGN), (dict(m=ADDR + 4), ALIGN), (dict(v=ADDR + 12), ALIGN),
    (dict(ema=ADDR + 4, ema_decay=0.5), ALIGN),
    (dict(off=None), ALIGN), (dict(length=None), ALIGN), (dict(seg=None), ALIGN), (dict(scale=None), ALIGN), (dict(wd=None), ALIGN),
    (dict(n_items=-1), SHAPE), (dict(n_seg=0), SHAPE), (dict(n_seg=-3), SHAPE), (dict(n_items=0, n_seg=0), SHAPE),
    (dict(beta1=1.0), UNSUPPORTED), (dict(beta1=-0.1), UNSUPPORTED), (dict(beta2=1.0), UNSUPPORTED), (dict(beta2=-0.5), UNSUPPORTED),
    (dict(beta1=float("nan")), UNSUPPORTED), (dict(beta2=float("nan")), UNSUPPORTED),
    (dict(ema=ADDR, ema_decay=1.0), UNSUPPORTED), (dict(ema=ADDR, ema_decay=-0.1), UNSUPPORTED),
    (dict(ema=ADDR, ema_decay=float("nan")), UNSUPPORTED), (dict(ema=ADDR, ema_decay=1.5, n_items=0), UNSUPPORTED),
    # nothing to do: success with no launch (these return before any kernel, or they could not succeed without a device)
    (dict(n_items=0), OK), (dict(n_items=0, ema=ADDR, ema_decay=0.999), OK), (dict(n_items=0, hyper=ADDR), OK),
    (dict(n_items=0, ema_decay=7.0), OK),                                       # without an ema array its decay is not looked at
    (dict(n_items=0, off=None, length=None, seg=None), OK),                     # an empty work list has no storage
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_adamw_table_argument_checks(kw, code):
    assert _call(**kw) == code


# ---------------------------------------------------------------- checkpoints
def test_checkpoint_keys_round_trip_on_cpu(tmp_path):
    from myrtle_vision.utils.models import load_checkpoint, save_checkpoint
    from myrtle_vision.utils.optim import CosineLRScheduler
    kw = dict(layer_decay=0.75, no_weight_decay=["pos_embedding", "cls_token"], ema_decay=0.99)
    vit = _vit("classification")
    opt = _table_opt(vit, **kw)
    opt.exp_avg.normal_()
    opt.step_count = 5
    opt.ema.add_(0.25)                                                          # an EMA that differs from the weights
    for o, p in zip(opt.arena.offsets, opt.arena.params):                       # (the gaps stay zero)
        opt.ema[o + p.numel():(o + p.numel() + 7) & ~7] = 0
    sched = CosineLRScheduler(opt, t_initial=10, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-6)
    sched.step(3)
    sd = opt.state_dict()
    assert sd["layer_decay"] == 0.75 and sd["no_weight_decay"] == ["pos_embedding", "cls_token"]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, 0.05]       # the two reference groups, torch's order
    assert sd["param_groups"][0]["lr"] == sd["param_groups"][1]["lr"] == opt.param_groups[0]["lr"]      # the BASE rate
    assert set(sd) == {"state", "param_groups", "param_names", "layer_decay", "no_weight_decay"}
    path = str(tmp_path / "vit_000005")
    save_checkpoint(vit, opt, sched, 5, path, model_ema=opt.ema_state_dict(vit))
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "lr_scheduler", "iteration", "model_ema"}
    assert list(ck["model_ema"].keys()) == list(vit.state_dict().keys())
    assert torch.equal(ck["model_ema"]["pos_embedding"], vit.pos_embedding.detach() + 0.25)
    vit2 = _vit("classification")
    opt2 = _table_opt(vit2, **kw)
    sched2 = CosineLRScheduler(opt2, t_initial=10, lr_min=1e-5, warmup_t=2, warmup_lr_init=1e-6)
    assert not opt2.ema_loaded
    assert load_checkpoint(vit2, opt2, sched2, path) == 5
    assert opt2.ema_loaded and torch.equal(opt2.ema, opt.ema) and torch.equal(opt2.arena.flat_param, opt.arena.flat_param)
    s1, s2 = sd["state"], opt2.state_dict()["state"]
    assert all(torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"]) for k in s1) and opt2.step_count == 5    # (arena padding is not state)
    assert opt2.param_groups[0]["lr"] == opt.param_groups[0]["lr"]
    # evaluation: use_ema loads "model_ema"; a checkpoint without it is an error that names the key
    vit3 = _vit("classification")
    load_checkpoint(vit3, None, None, path, use_ema=True)
    assert torch.equal(vit3.pos_embedding.detach(), ck["model_ema"]["pos_embedding"])
    plain = str(tmp_path / "plain")
    save_checkpoint(vit, opt, sched, 5, plain)
    assert set(torch.load(plain, map_location="cpu", weights_only=False)) == {"model", "optimizer", "lr_scheduler", "iteration"}
    with pytest.raises(KeyError, match="model_ema"):
        load_checkpoint(_vit("classification"), None, None, plain, use_ema=True)
    # another recipe refuses the checkpoint
    for other in (dict(layer_decay=0.65, no_weight_decay=["pos_embedding", "cls_token"]), dict(layer_decay=0.75),
                  dict(no_weight_decay=["pos_embedding", "cls_token"])):
        with pytest.raises(ValueError, match="layer_decay|no_weight_decay"):
            _table_opt(_vit("classification"), **other).load_state_dict(sd)
    from myrtle_vision.utils.optim import AdamW, ParamArena
    v4 = _vit("classification")
    AdamW(ParamArena(v4.named_parameters(), skip=v4.unused_parameter_names()), lr=1e-3, weight_decay=0.05).load_state_dict(sd)


def test_step_refuses_two_learning_rates_and_the_ema_context_on_cpu():
    """Both answers come before any kernel, so they can be asked without a device."""
    opt = _table_opt(_vit("classification"), ema_decay=0.9)
    opt.param_groups[1]["lr"] = 5e-4
    with pytest.raises(ValueError, match="learning rate"):
        opt.step()
    opt.param_groups[1]["lr"] = opt.param_groups[0]["lr"]
    p0, e0 = opt.arena.flat_param.clone(), (opt.ema.add_(1.0)).clone()
    with opt.ema_weights():
        assert torch.equal(opt.arena.flat_param, e0) and torch.equal(opt.ema, p0)
        with pytest.raises(RuntimeError, match="ema_weights"):
            opt.step()
    assert torch.equal(opt.arena.flat_param, p0) and torch.equal(opt.ema, e0)
    with pytest.raises(RuntimeError, match="ema_decay"):
        _table_opt(_vit("classification"), layer_decay=0.75).ema_weights().__enter__()
